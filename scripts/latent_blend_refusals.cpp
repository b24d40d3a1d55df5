// Stand-alone host program: every refusal of slh_latent_blend (include/sliders_hip.h), called with addresses that are never
// dereferenced - each call must be refused before any launch, so no device is needed.  Built with the host sanitizers
// (make -C sliders_amd/csrc latent_blend_refusals, then run build/latent_blend_refusals): AddressSanitizer and
// UndefinedBehaviorSanitizer see the entry point's own host code (argument reads, alignment and overlap arithmetic, the message
// formatting of slh_set_error).  Exit status 0: every case was refused with a message that names it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/sliders_hip.h"

static int failures = 0;

static void refused(const char* what, const void* const* ptrs, const int32_t* dims, const float* coef) {
    const int rc = slh_latent_blend(ptrs, dims, coef, nullptr);
    const char* msg = slh_last_error();
    const bool ok = rc != 0 && msg && strstr(msg, "slh_latent_blend") && strstr(msg, what);
    printf("%-28s rc %d  %s\n", what, rc, msg ? msg : "(no message)");
    if (!ok) ++failures;
}

int main() {
    const auto P = [](uintptr_t v) { return (const void*)v; };
    const float one[1] = {1.0f};
    const float inf[1] = {std::numeric_limits<float>::infinity()};
    const float nan[1] = {std::nanf("")};
    const int32_t bf16[4] = {1, 64, 16, 0}, fp32[4] = {1, 64, 16, 1};
    const void* ok[6] = {P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000), P(0x6000)};
    refused("null ptrs / dims", nullptr, fp32, one);
    refused("null ptrs / dims", ok, nullptr, one);
    for (int hole = 0; hole < 4; ++hole) {
        const void* p[6];
        memcpy(p, ok, sizeof p);
        p[hole] = nullptr;
        refused("null e / keep / mask / out", p, fp32, one);
        refused("null e / keep / mask / out", p, bf16, nullptr);
    }
    for (int k = 0; k < 3; ++k) {          // nb, chw, hw below 1
        for (int32_t bad : {0, -3}) {
            int32_t d[4] = {1, 64, 16, 1};
            d[k] = bad;
            refused(k == 0 ? "nb = " : k == 1 ? "chw = " : "hw = ", ok, d, one);
        }
    }
    { const int32_t d[4] = {1, 64, 24, 1}; refused("not a multiple of hw", ok, d, one); }
    { const int32_t d[4] = {1, 64, 16, 2}; refused("dtype 2", ok, d, one); }
    { const int32_t d[4] = {1, 64, 16, -1}; refused("dtype -1", ok, d, one); }
    refused("needs coef", ok, fp32, nullptr);
    refused("is not finite", ok, fp32, inf);
    refused("is not finite", ok, fp32, nan);
    for (int k : {0, 1, 3}) {              // e / keep / out
        const void* p[6];
        memcpy(p, ok, sizeof p);
        p[k] = P((uintptr_t)ok[k] + 2);
        refused("not 4-byte aligned", p, fp32, one);
        p[k] = P((uintptr_t)ok[k] + 1);
        refused("not 2-byte aligned", p, bf16, one);
    }
    for (int k : {4, 5}) {
        const void* p[6];
        memcpy(p, ok, sizeof p);
        p[k] = P((uintptr_t)ok[k] + 1);
        refused("not 2-byte aligned", p, fp32, one);
    }
    { const void* p[6]; memcpy(p, ok, sizeof p); p[2] = P(0x3002); refused("mask pointer", p, bf16, one); }
    { const void* p[6]; memcpy(p, ok, sizeof p); p[1] = P(0x4080); refused("keep overlaps out", p, fp32, one); }
    { const void* p[6]; memcpy(p, ok, sizeof p); p[2] = P(0x5010); refused("mask overlaps in_bf16", p, fp32, one); }
    { const void* p[6]; memcpy(p, ok, sizeof p); p[1] = P(0x6040); refused("keep overlaps in2_bf16", p, bf16, one); }
    printf(failures ? "FAILED: %d case(s) not refused as expected\n" : "all refused\n", failures);
    return failures ? 1 : 0;
}
