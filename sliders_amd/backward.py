"""Backward through the frozen net into the LoRA adapters (loss.backward(), train_lora_xl.py:345): the reverse walk over the tape
of a train-mode UNetPlan.  It shares with the forward walk the plan skeleton (planner.Plan), the tape's record types and the
descriptor helpers - nothing else."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import lib
from .planner import (Act, AttnRec, ConvOutRec, GegluRec, GemmRec, GnRec, LnRec, Plan, UNetPlan, conv_fields, head_t, sources,
                      src_parts)
from .tuning import choose_tile


class BackwardPlan(Plan):
    """Reverse walk over a train-mode UNetPlan's tape.  Gradients flow only for samples [b0, b0+nb): in the
    reference's CFG pair the unconditional half receives an exactly-zero gradient (d/du of u + 1*(t-u) is
    1 - 1 = 0 in bf16, train_util.py:250-253 with guidance_scale=1), so its backward is skipped.

    Every backward-data product reuses slh_gemm with the pre-transposed frozen weights; LoRA gradients are
    skinny reductions (slh_skinny with the up matrix as a [K][4] down-projection of dY, slh_lora_wgrad)."""

    def __init__(self, fwd: UNetPlan, b0: int, nb: int, one_ptr: int):
        assert fwd.train and fwd.lora is not None
        super().__init__(fwd.w, fwd.arena, fwd.zarena, fwd.sw)      # one environment for a forward plan and its backward
        self.f = fwd
        self.cfg, self.lora = fwd.cfg, fwd.lora
        self.b0, self.nb = b0, nb
        self.one_ptr = one_ptr
        self.scale_ptr = fwd.lora_scale_ptr
        self._g: Dict[int, Act] = {}          # base buffer ptr -> full-width gradient buffer (nb samples)
        self._written = set()
        H, W = fwd.H, fwd.W
        self.deps_pix = self.arena.alloc((nb * H * W, 4), torch.float32, "bwd.deps_pix")
        # launches that do not sit on the dependency chain are collected and issued as ONE batched launch each
        # (slh_batch_desc): the head transposes of FORWARD activations (K^T, Q^T of every attention layer) at the head of the
        # program, and the adapters' weight gradients at its tail - except the up-gradient (dB) of a module whose output
        # gradient buffer doubles as its residual input's (alias_grad): later accumulations would change dY under it
        # dO^T of a self-attention (for dK / dV) comes out of the backward-data product that produces dO (vt_out + vt_also_c)
        # instead of a transpose launch: attention output buffer -> (heads, Tq), filled from the tape; -> (buffer, ldt) once made
        self._wants_dot: Dict[int, Tuple[int, int]] = {}
        self._dot_made: Dict[int, Tuple] = {}
        # GEGLU outputs -> their tape record: the backward-data product of the Linear that consumes one writes d(proj) itself
        self._geglu_of: Dict[int, GegluRec] = {}
        for rec in fwd.tape:
            if isinstance(rec, AttnRec) and rec.k.buf.ptr not in fwd.nograd_kv and not self.sw.bwd_dot_launch:
                self._wants_dot[rec.o.buf.ptr] = (rec.heads, rec.q.HW)
            if isinstance(rec, GegluRec) and not self.sw.bwd_unfused_geglu:
                self._geglu_of[rec.out.buf.ptr] = rec
        self._tr_batch: List = []
        self._wg_batch: Dict[int, List] = {4: [], 12: []}
        self._keep: List = []            # device tables of the batched launches
        self.batched = not self.sw.bwd_unbatched
        # weight gradients reduced over their M splits in a fixed order (slabs + tickets) instead of fp32 atomics: the LoRA
        # gradient buffer is bit-reproducible.  SLIDERS_WGRAD_ATOMIC=1: the old form (A/B)
        self.wgrad_fixed_order = not self.sw.wgrad_atomic
        self.fuse_u = not self.sw.bwd_unfused_u
        self._uses_up_t = False
        self._walk()
        dev = None if self.arena.virtual else fwd.lora.params.device
        for R, descs in self._wg_batch.items():
            if descs:
                if self.wgrad_fixed_order:
                    for d in descs:
                        d.slabs = 8                 # marker: slab geometry (the workspace is the batch's)
                bd, keep = lib.batch_table(lib.OP_WGRAD_BATCH, descs, dev, arg=R)
                if self.wgrad_fixed_order:
                    # one slab of 256 R floats and one ticket per workgroup: the M splits of a column block meet in a fixed order
                    bd.slabs = self.arena.alloc((bd.total, 256 * R), torch.float32, f"bwd.wgrad_slabs_R{R}").ptr
                    bd.tickets = self.zarena.alloc((bd.total,), torch.int32, f"bwd.wgrad_tickets_R{R}").ptr
                self._keep.append(keep)
                self.add(lib.OP_WGRAD_BATCH, bd, f"bwd.wgrad_batch_R{R}")
        head = []
        if self._uses_up_t:
            if self.arena.virtual:
                gd = lib.Gather16Desc(src=0x1000, idx=0x1000, out=0x1000, n=1)
            else:
                gd = lib.Gather16Desc(src=fwd.lora.params.data_ptr(), idx=fwd.lora.up_t_index.data_ptr(),
                                      out=fwd.lora.up_t.data_ptr(), n=fwd.lora.up_t.numel())
            head.append((lib.OP_GATHER16, gd, "bwd.up_t"))
        if self._tr_batch:
            bd, keep = lib.batch_table(lib.OP_TRANSPOSE_BATCH, self._tr_batch, dev)
            self._keep.append(keep)
            head.append((lib.OP_TRANSPOSE_BATCH, bd, "bwd.kt_qt_batch"))
        self.put_head("zero_bwd_stats", head)
        self.prog = self.program()

    # ---- gradient buffers ------------------------------------------------------------------------
    def _sl(self, a: Act) -> Act:
        return a.sample(self.b0, self.nb)

    def grad(self, a: Act, write: bool = True):
        """(gradient view matching `a` for the selected samples, accumulate?)"""
        base = a.buf.ptr
        g = self._g.get(base)
        if g is None:
            rows = self.nb * a.HW
            buf = self.arena.alloc((rows, a.ld), torch.bfloat16, "g:" + a.name)
            g = Act(buf.ptr, self.nb, a.H, a.W, a.ld, a.ld, buf, "g:" + a.name)
            self._g[base] = g
        c0 = ((a.ptr - a.buf.ptr) // 2) % a.ld
        view = Act(g.ptr + 2 * c0, self.nb, a.H, a.W, a.C, g.ld, g.buf, g.name)
        key = (base, c0, a.C)
        acc = key in self._written
        if write:
            self._written.add(key)
        return view, acc

    def has_grad(self, a: Act) -> bool:
        """True once any column range of a's buffer has received a gradient."""
        return any(k[0] == a.buf.ptr for k in self._written)

    def alias_grad(self, a: Act, g: Act):
        self._g[a.buf.ptr] = Act(g.ptr, g.B, g.H, g.W, a.ld, g.ld, g.buf, g.name)
        self._written.add((a.buf.ptr, 0, a.C))

    # ---- op emitters -----------------------------------------------------------------------------
    def _ew(self, op, a: Act, out: Act, b: Optional[Act] = None, name="", C=None, iarg=0, iarg2=0, M=None):
        d = lib.EwDesc(a=a.ptr, b=b.ptr if b else 0, out=out.ptr, M=M if M is not None else a.M, C=C or a.C, lda=a.ld,
                       ldb=b.ld if b else 0, ldo=out.ld, op=op, iarg=iarg, iarg2=iarg2)
        self.add(lib.OP_ELEMENTWISE, d, name)

    def add_into(self, dst_fwd: Act, src: Act, name: str):
        g, acc = self.grad(dst_fwd)
        if acc:
            self._ew(lib.EW_ADD, g, g, src, name + ".add")
        else:
            self._ew(lib.EW_COPY, src, g, name=name + ".copy")

    def _walk(self):
        for rec in reversed(self.f.tape):
            handler = self.HANDLERS.get(type(rec))
            if handler is None:
                raise TypeError(f"the backward has no handler for a tape record of kind {type(rec).__name__}")
            handler(self, rec)

    def _b_conv_out(self, rec: ConvOutRec):
        x = rec.x
        gx, acc = self.grad(x)
        d = lib.LoraCdgradDesc(u=self.deps_pix.ptr, a_down=self.w.ptr("conv_out.w"), scale=self.one_ptr, gx=gx.ptr,
                               batch=self.nb, hl=x.H, wl=x.W, ho=x.H, wo=x.W, stride=1, cin=x.C, ldu=4, ldgx=gx.ld,
                               accumulate=1 if acc else 0)
        self.add(lib.OP_LORA_CONV_DGRAD, d, "bwd.conv_out")

    def _b_gn(self, rec: GnRec):
        x0, x1 = src_parts(rec.x)
        y = rec.out
        if not self.has_grad(y):
            return
        need0 = x0.buf.ptr not in self.f.nograd
        need1 = x1 is not None and x1.buf.ptr not in self.f.nograd
        if not (need0 or need1):
            return
        gy, _ = self.grad(y, write=False)
        G = self.cfg.norm_num_groups
        bst = self.arena.alloc((self.nb, G, 2), torch.float32, "bwd." + rec.name + ".bstats")
        prow, ntick = lib.gn_workspace(x0.C + (x1.C if x1 is not None else 0), x0.HW, G)
        bpart = self.arena.alloc((self.nb, prow, G, 2), torch.float32, "bwd." + rec.name + ".bpartial")
        btick = self.zarena.alloc((self.nb, ntick), torch.float32, "bwd." + rec.name + ".bticket")
        x0s = self._sl(x0)
        x1s = self._sl(x1) if x1 is not None else None
        g0, a0 = self.grad(x0) if need0 else (None, False)
        g1, a1 = self.grad(x1) if need1 else (None, False)
        st = rec.stats.ptr + 4 * self.b0 * G * 2
        d = lib.GnBwdDesc(**sources(x0s, x1s, "x", "ldx", "c"), gamma=self.w.ptr(rec.wname + ".g"),
                          beta=self.w.ptr(rec.wname + ".b"), stats=st, bstats=bst.ptr, dy=gy.ptr,
                          dx0=g0.ptr if g0 else 0, dx1=g1.ptr if g1 else 0, batch=self.nb, hw=x0.HW, groups=G, lddy=gy.ld,
                          lddx0=g0.ld if g0 else 0, lddx1=g1.ld if g1 else 0, eps=rec.eps, act=rec.act,
                          accumulate0=1 if a0 else 0, accumulate1=1 if a1 else 0, bpartial=bpart.ptr, bticket=btick.ptr)
        self.add(lib.OP_GN_BWD_STATS, d, "bwd." + rec.name + ".stats")
        self.add(lib.OP_GN_BWD_APPLY, d, "bwd." + rec.name + ".apply")

    def _b_ln(self, rec: LnRec):
        x, y = rec.x, rec.out
        if not self.has_grad(y):
            return
        gy, _ = self.grad(y, write=False)
        gx, acc = self.grad(x)
        xs = self._sl(x)
        mr = rec.mr.ptr + 4 * 2 * self.b0 * x.HW
        d = lib.LnBwdDesc(x=xs.ptr, gamma=self.w.ptr(rec.wname + ".g"), dy=gy.ptr, mean_rstd=mr, dx=gx.ptr,
                          M=xs.M, C=x.C, ldx=xs.ld, lddy=gy.ld, lddx=gx.ld, accumulate=1 if acc else 0)
        self.add(lib.OP_LAYERNORM_BWD, d, "bwd." + rec.name)

    def _b_geglu(self, rec: GegluRec):
        pre, out = rec.pre, rec.out
        if not self.has_grad(out):
            return
        go, _ = self.grad(out, write=False)
        gp, acc = self.grad(pre)
        assert not acc
        ps = self._sl(pre)
        self._ew(lib.EW_GEGLU_BWD, ps, gp, go, "bwd." + rec.name, C=out.C)

    def _transpose(self, src: Act, heads: int, T: int, name: str, forward_data: bool = False):
        """forward_data: src is an activation of the forward pass (final before the backward starts): the transpose joins
        the one batched launch at the head of the program instead of sitting in the chain."""
        D = src.C // heads
        Dp, ldt = head_t(D, T)
        t = self.arena.alloc((self.nb, heads, Dp, ldt), torch.bfloat16, name)
        d = lib.TransposeDesc(src=src.ptr, dst=t.ptr, B=self.nb, H=heads, T=T, ld=src.ld, ldt=ldt, D=D)
        if forward_data and self.batched:
            self._tr_batch.append(d)
        else:
            self.add(lib.OP_TRANSPOSE_HEADS, d, name)
        return t, ldt

    def _b_attn(self, rec: AttnRec):
        q, k, v, o = rec.q, rec.k, rec.v, rec.o
        if not self.has_grad(o):
            return
        heads, Tk, Tq = rec.heads, rec.Tk, q.HW
        go, _ = self.grad(o, write=False)
        need_dkv = 1 if (k.buf.ptr not in self.f.nograd_kv) else 0
        qs, ks, vs, os_ = self._sl(q), self._sl(k), self._sl(v), self._sl(o)
        kt, ldkt = self._transpose(ks, heads, Tk, "bwd." + rec.name + ".kt", forward_data=True)
        gq, aq = self.grad(q)
        assert not aq
        delta = self.arena.alloc((self.nb * heads * Tq + 64,), torch.float32, "bwd." + rec.name + ".delta")
        d = lib.AttnBwdDesc(q=qs.ptr, k=ks.ptr, v=vs.ptr, o=os_.ptr, d_o=go.ptr, kt=kt.ptr,
                            lse=rec.lse.ptr + 4 * self.b0 * heads * Tq, delta=delta.ptr, dq=gq.ptr,
                            B=self.nb, H=heads, Tq=Tq, Tk=Tk, ldq=qs.ld, ldk=ks.ld, ldv=vs.ld, ldo=os_.ld, lddo=go.ld,
                            ldkt=ldkt, lddq=gq.ld, scale=(q.C // heads) ** -0.5, need_dkv=need_dkv, D=q.C // heads)
        if need_dkv:
            qt, ldqt = self._transpose(qs, heads, Tq, "bwd." + rec.name + ".qt", forward_data=True)
            made = self._dot_made.get(o.buf.ptr)
            if made is not None:
                dot = made[0]                 # written head-transposed by the product that produced dO
                assert made[1] == ldqt
            else:
                dot, _ = self._transpose(go, heads, Tq, "bwd." + rec.name + ".dot")
            gk, ak = self.grad(k)
            gv, av = self.grad(v)
            assert not ak and not av
            d.qt, d.dot, d.ldqt, d.dk, d.dv, d.lddk, d.lddv = qt.ptr, dot.ptr, ldqt, gk.ptr, gv.ptr, gk.ld, gv.ld
        self.add(lib.OP_ATTN_BWD, d, "bwd." + rec.name)

    def _tile(self, d, name, vt=None):
        choose_tile(d, vt=vt, backward=True)
        self.provision_splitk(d, name)

    def _wgrad(self, d, name: str, defer: bool):
        if defer and self.batched:
            self._wg_batch[d.R].append(d)
        else:
            if self.wgrad_fixed_order:
                nb = lib.wgrad_single_blocks(d)
                d.slabs = self.arena.alloc((nb, 256 * d.R), torch.float32, name + ".slabs").ptr
                d.tickets = self.zarena.alloc((nb,), torch.int32, name + ".tickets").ptr
            self.add(lib.OP_WGRAD, d, name)

    def _b_gemm(self, rec: GemmRec):
        y = rec.out
        if not self.has_grad(y):
            return
        name = "bwd." + rec.name
        gy, _ = self.grad(y, write=False)
        x0, x1 = src_parts(rec.x)
        need0 = x0.buf.ptr not in self.f.nograd
        need1 = x1 is not None and x1.buf.ptr not in self.f.nograd
        self._b_gemm_residual(rec, gy, name)
        if rec.temb_path and self.lora.temb_entries:
            self._b_gemm_temb(rec, gy, name)
        U, up_t_off, dA_after = self._b_gemm_lora(rec, gy, name, need0 or need1) if rec.grp is not None else (None, None, [])
        if not (need0 or need1):
            return
        if rec.conv is None:
            self._b_gemm_linear(rec, gy, name, need0, need1, U, up_t_off, dA_after)
        else:
            self._b_gemm_conv(rec, gy, name, U)

    def _b_gemm_residual(self, rec: GemmRec, gy: Act, name: str):
        """residual branch: d(out)/d(residual) = identity"""
        r = rec.residual
        if r is not None and r.buf.ptr not in self.f.nograd:
            if r.buf.ptr not in self._g and r.ld == r.C and gy.ld == gy.C and r.C == gy.C:
                self.alias_grad(r, gy)
            else:
                self.add_into(r, gy, name + ".res")

    def _b_gemm_temb(self, rec: GemmRec, gy: Act, name: str):
        """time-embedding add: gradient w.r.t. the per-sample bias feeds the time_emb_proj adapter"""
        f, N = self.f, rec.N
        i = f.w.resnet_paths.index(rec.temb_path)
        e = self.lora.temb_entries[i]
        gsum = self.zarena.alloc((self.nb, N), torch.float32, name + ".gtemb")
        self._ew(lib.EW_COLSUM, gy, Act(gsum.ptr, self.nb, 1, 1, N, N, gsum), name=name + ".colsum", iarg2=rec.Ho * rec.Wo)
        ted = self.cfg.time_embed_dim
        L4 = f.temb_lora_T.shape[1]
        for s in range(self.nb):
            d = lib.TembLoraBwdDesc(g=gsum.ptr + 4 * s * N, t=f.temb_lora_T.ptr + 4 * ((self.b0 + s) * L4 + 4 * i),
                                    up=self.lora.up_ptr(e), emb=f.emb.ptr + 2 * (self.b0 + s) * ted,
                                    d_up=self.lora.gup_ptr(e), d_down=self.lora.gdown_ptr(e), scale=self.scale_ptr,
                                    C=N, ted=ted)
            self.add(lib.OP_TEMB_LORA_BWD, d, name + ".temb_lora")

    def _b_gemm_lora(self, rec: GemmRec, gy: Act, name: str, dgrad: bool):
        """LoRA: U = dY . B_up per fused member; dB = s dY^T T ; dA = s U^T X.  dgrad: a backward-data product follows.  Returns
        (U, the offset of the group's k-major up matrices when U comes out of that product - else None -, the down-gradients that
        must wait for it)."""
        f = self.f
        x0, x1 = src_parts(rec.x)
        conv, grp, N, K, r, Ho, Wo = rec.conv, rec.grp, rec.N, rec.K, rec.residual, rec.Ho, rec.Wo
        Ms = self.nb * Ho * Wo
        dA_after = []
        ng = len(grp)
        Ng = N // ng
        U = self.arena.alloc((Ms, 4 * ng), torch.float32, name + ".U")
        Ts = rec.T.ptr + 4 * self.b0 * (Ho * Wo) * 4 * ng
        # U = dY . B (the up matrices as a rank-4 down-projection of the output gradient): inside the backward-data GEMM
        # of a dense module - third operand tile = the k-major copy of B (LoraStore.up_t), written out through lora_t_out
        # for the down-gradient - unless that product does not exist (no gradient needed upstream)
        up_t_off = self.lora.up_t_offset(grp) if (self.fuse_u and conv is None and x1 is None and dgrad) else None
        fused_u = up_t_off is not None          # (split-K included: the slice that arrives last reduces T as well)
        if not fused_u:
            for g_i, e in enumerate(grp):
                d = lib.SkinnyDesc(a0=gy.ptr + 2 * g_i * Ng, w=self.lora.up_ptr(e), out=U.ptr + 4 * 4 * g_i, lda0=gy.ld,
                                   ca0=Ng, mode=0, stride=1, M=Ms, R=4, K=Ng, ldo=4 * ng, w_kmajor=1)
                self.add(lib.OP_SKINNY, d, name + f".U{g_i}")
        d = lib.WgradDesc(z0=gy.ptr, v=Ts, out=self.lora.gup_ptr(grp[0]), scale=self.scale_ptr, ldz0=gy.ld, c0=N,
                          mode=0, stride=1, M=Ms, R=4, ldv=4 * ng, ldo=4, out_rmajor=0,
                          vgroup_cols=Ng if ng > 1 else 0)
        # dY of a module with a residual input may be the residual's gradient buffer too (alias_grad above): it keeps
        # accumulating after this point, so its up-gradient cannot wait for the batched launch at the tail
        self._wgrad(d, name + ".dB", defer=r is None or r.buf.ptr in f.nograd)
        x0s = self._sl(x0)
        x1s = self._sl(x1) if x1 is not None else None
        # the down matrices of a fused q|k|v group are adjacent ([12][K]) and so are their U columns: one R = 12 launch
        # reads X once instead of three times
        one = ng == 3 and conv is None
        for g_i, e in enumerate(grp[:1] if one else grp):
            d = lib.WgradDesc(**sources(x0s, x1s, "z", "ldz", "c"), v=U.ptr + 4 * 4 * g_i, out=self.lora.gdown_ptr(e),
                              scale=self.scale_ptr, mode=0, stride=1, M=Ms, R=12 if one else 4, ldv=4 * ng,
                              ldo=K, out_rmajor=1, vgroup_cols=0)
            if conv is not None:
                conv_fields(d, conv, x0s, Ho, Wo)
            if fused_u:
                dA_after.append((d, name + f".dA{g_i}"))            # U is written by the dgrad launch below
            else:
                self._wgrad(d, name + f".dA{g_i}", defer=True)      # forward activations and U: final
        return U, up_t_off, dA_after

    def _b_gemm_linear(self, rec: GemmRec, gy: Act, name: str, need0: bool, need1: bool, U, up_t_off, dA_after):
        """backward data of a Linear / 1x1 convolution"""
        x0, x1 = src_parts(rec.x)
        grp, N, Ho, Wo = rec.grp, rec.N, rec.Ho, rec.Wo
        Ms = self.nb * Ho * Wo
        cin = x0.C + (x1.C if x1 is not None else 0)
        wT = self.w.ptr(rec.wname + ".wT")
        geglu_rec = self._geglu_of.get(x0.buf.ptr) if (x1 is None and grp is None and not self.has_grad(x0)) else None
        if geglu_rec is not None and x0.C % 32 == 0:
            # the Linear behind a GEGLU (ff.net.2): its backward-data product writes d(proj) directly (GEGLU backward in
            # the epilogue, slh_gemm_desc.geglu = 2) - no d(ff) tensor, no elementwise launch
            pre = geglu_rec.pre
            gp, pacc = self.grad(pre)
            assert not pacc
            ps = self._sl(pre)
            d = lib.GemmDesc(a0=gy.ptr, w=wT, c=gp.ptr, lda0=gy.ld, ca0=N, mode=0, stride=1, ldw=N, M=Ms, N=cin, K=N,
                             ldc=gp.ld, rows_per_sample=Ho * Wo, geglu=2, geglu_pre=ps.ptr, ld_pre=ps.ld,
                             w_layout=self.w_layout)
            self._tile(d, name)
            self.add(lib.OP_GEMM, d, name + ".dgrad")
            return
        if x1 is None:
            gx, acc = self.grad(x0)
            tgt, tacc = gx, acc
        else:
            tb = self.arena.alloc((Ms, cin), torch.bfloat16, name + ".gxcat")
            tgt, tacc = Act(tb.ptr, self.nb, x0.H, x0.W, cin, cin, tb), False
        d = lib.GemmDesc(a0=gy.ptr, w=wT, c=tgt.ptr, residual=tgt.ptr if tacc else 0, lda0=gy.ld, ca0=N, mode=0,
                         stride=1, ldw=N, M=Ms, N=cin, K=N, ld_res=tgt.ld, ldc=tgt.ld, rows_per_sample=Ho * Wo,
                         w_layout=self.w_layout)
        if grp is not None:
            d.ld_t, d.lora_up, d.lora_scale = 4 * len(grp), self.lora.down_ptr(grp[0]), self.scale_ptr
            d.lora_groups, d.lora_rank, d.lora_up_rmajor = 1, 4 * len(grp), 1
            if up_t_off is not None:
                self._uses_up_t = True
                base = 0x2000 if self.arena.virtual else self.lora.up_t.data_ptr()
                d.lora_down, d.lora_t_out = base + 2 * up_t_off, U.ptr
            else:
                d.lora_t = U.ptr
        want = self._wants_dot.get(x0.buf.ptr) if (x1 is None and not tacc and tgt.ptr == gx.ptr) else None
        vt = None
        if want is not None:
            heads, Tq = want
            Dh = cin // heads
            if Dh % 64 == 0 and Tq % 64 == 0 and Ms == self.nb * Tq and cin == x0.C and tgt.ld % 8 == 0:
                vt = dict(vt_col0=0, vt_D=Dh, vt_heads=heads, vt_tokens=Tq, vt_ld=Tq, vt_also_c=1)
        self._tile(d, name, vt)
        if d.vt_out:
            dot = self.arena.alloc((self.nb, heads, Dh, Tq), torch.bfloat16, name + ".dot")
            d.vt_out = dot.ptr
            self._dot_made[x0.buf.ptr] = (dot, Tq)
        self.add(lib.OP_GEMM, d, name + ".dgrad")
        for dA, nm in dA_after:
            self._wgrad(dA, nm, defer=True)
        if x1 is not None:
            if need0:
                self.add_into(x0, tgt.cols(0, x0.C), name + ".gx0")
            if need1:
                self.add_into(x1, tgt.cols(x0.C, x1.C), name + ".gx1")

    def _b_gemm_conv(self, rec: GemmRec, gy: Act, name: str, U):
        """backward data of a 3x3 convolution"""
        x0, x1 = src_parts(rec.x)
        conv, grp, N, Ho, Wo = rec.conv, rec.grp, rec.N, rec.Ho, rec.Wo
        cin = x0.C
        wT = self.w.ptr(rec.wname + ".wT")
        assert x1 is None
        if conv.xform == 1:     # forward read a nearest-2x upsampled image: dgrad lands on the 2h x 2w grid first
            HL, WL = 2 * x0.H, 2 * x0.W
            tb = self.arena.alloc((self.nb * HL * WL, cin), torch.bfloat16, name + ".gx_up")
            tgt, tacc = Act(tb.ptr, self.nb, HL, WL, cin, cin, tb), False
        else:
            HL, WL = x0.H, x0.W
            tgt, tacc = self.grad(x0)
        d = lib.GemmDesc(a0=gy.ptr, w=wT, c=tgt.ptr, residual=tgt.ptr if tacc else 0, lda0=gy.ld, ca0=N, mode=1,
                         batch=self.nb, hs=Ho, ws=Wo, src_xform=2 if conv.stride == 2 else 0, stride=1, ho=HL, wo=WL,
                         ldw=9 * N, M=self.nb * HL * WL, N=cin, K=9 * N, ld_res=tgt.ld, ldc=tgt.ld,
                         rows_per_sample=HL * WL, w_layout=self.w_layout)
        self._tile(d, name)
        self.add(lib.OP_GEMM, d, name + ".dgrad")
        if grp is not None:
            d2 = lib.LoraCdgradDesc(u=U.ptr, a_down=self.lora.down_ptr(grp[0]), scale=self.scale_ptr, gx=tgt.ptr,
                                    batch=self.nb, hl=HL, wl=WL, ho=Ho, wo=Wo, stride=conv.stride, cin=cin, ldu=4,
                                    ldgx=tgt.ld, accumulate=1)
            self.add(lib.OP_LORA_CONV_DGRAD, d2, name + ".lora_dgrad")
        if conv.xform == 1:
            gx, acc = self.grad(x0)
            if acc:
                t2b = self.arena.alloc((self.nb * x0.HW, cin), torch.bfloat16, name + ".gx_dn")
                t2 = Act(t2b.ptr, self.nb, x0.H, x0.W, cin, cin, t2b)
                self._ew(lib.EW_UPSAMPLE_BWD, tgt, t2, name=name + ".upsample_bwd", iarg=x0.W, iarg2=x0.HW, M=t2.M)
                self._ew(lib.EW_ADD, gx, gx, t2, name + ".add")
            else:
                self._ew(lib.EW_UPSAMPLE_BWD, tgt, gx, name=name + ".upsample_bwd", iarg=x0.W, iarg2=x0.HW, M=gx.M)

    HANDLERS = {GemmRec: _b_gemm, GnRec: _b_gn, LnRec: _b_ln, AttnRec: _b_attn, GegluRec: _b_geglu, ConvOutRec: _b_conv_out}
