// last-error string + version for libsliders_hip.so
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include "../../include/sliders_hip.h"

static thread_local char g_err[512] = "";

void slh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* slh_last_error(void) { return g_err; }
extern "C" int slh_version(void) { return 2; }

// ---- launch query (slh_gemm_kernel_name, slh_gemm_launch_query) ----------------------------------------------------------------
// While a sink is set on this thread the launchers (common.h: slh_launch<Kern>) record the instantiation they WOULD launch instead of
// launching it: the name is formatted at the launch site from the template arguments themselves, in rocprofv3's spelling, and the
// grid, the block size and a 64-bit FNV-1a hash of the argument struct's bytes are kept beside it.
#include <string.h>
static thread_local char* g_name_sink = nullptr;
static thread_local int g_name_cap = 0;

bool slh_name_mode() { return g_name_sink != nullptr; }
static thread_local int g_rec_grid = 0, g_rec_block = 0;
static thread_local unsigned long long g_rec_hash = 0;
void slh_name_sink_set(char* buf, int cap) {
    g_name_sink = buf; g_name_cap = cap;
    if (buf && cap > 0) { buf[0] = 0; g_rec_grid = g_rec_block = 0; g_rec_hash = 0; }
}

void slh_launch_record(int grid, int block, const void* args, size_t bytes) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char*)args)[i]) * 0x100000001b3ull;
    g_rec_grid = grid; g_rec_block = block; g_rec_hash = h;
}
void slh_launch_recorded(int* grid, int* block, unsigned long long* args_hash) {
    *grid = g_rec_grid; *block = g_rec_block; *args_hash = g_rec_hash;
}

void slh_name_record(const char* fmt, ...) {
    if (!g_name_sink || g_name_cap <= 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_name_sink, g_name_cap, fmt, ap);
    va_end(ap);
}
