"""Backward parity: attention backward and the LoRA-gradient helpers against torch autograd (fp32) on the same
bf16-rounded inputs, then the whole UNet backward (d loss / d LoRA parameters) of the HIP engine against
autograd through the CPU oracle + oracle LoRA (= what loss.backward() does in the reference,
trainscripts/textsliders/train_lora_xl.py:345).

Tolerances: bf16 gradients chained through ~100 layers; the engine must be as close to the fp32 oracle as
the reference-precision arm (oracle run in torch bf16): rel_l2(engine) <= rel_l2(bf16 arm) + 1e-3 on the
flat gradient vector, and cosine similarity with the fp32 gradient >= 0.999.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle.lora_oracle import LoRANetworkOracle
from oracle.unet_oracle import build_unet
from sliders_amd import lib
from sliders_amd.config import CONFIGS
from sliders_amd.lora_store import LoraStore
from sliders_amd.unet import UNetEngine
from tests.test_unet_gpu import make_inputs
from tests.util import bf, p, rel_err, report, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,Tq,Tk,dkv,D", [(1, 3, 256, 256, 1, 64), (2, 2, 192, 192, 1, 64), (1, 4, 320, 77, 0, 64),
                                              (1, 2, 100, 77, 1, 64), (1, 8, 256, 256, 1, 40), (1, 4, 128, 77, 1, 80),
                                              (1, 8, 64, 64, 1, 160), (1, 2, 200, 77, 0, 160), (1, 4, 96, 96, 1, 16)])
def test_attention_bwd(dev, B, H, Tq, Tk, dkv, D):
    torch.manual_seed(21)
    C = H * D
    sc = D ** -0.5
    q = bf(torch.randn(B * Tq, C, device=dev))
    k = bf(torch.randn(B * Tk, C, device=dev))
    v = bf(torch.randn(B * Tk, C, device=dev))
    go = bf(torch.randn(B * Tq, C, device=dev))

    def tr(x, T):
        ldt = (T + 63) // 64 * 64
        t = torch.zeros(B, H, (D + 63) // 64 * 64, ldt, device=dev, dtype=torch.bfloat16)
        lib.call(lib.OP_TRANSPOSE_HEADS, lib.TransposeDesc(src=p(x), dst=p(t), B=B, H=H, T=T, ld=C, ldt=ldt, D=D), stream())
        return t, ldt

    vt, ldvt = tr(v, Tk)
    o = torch.zeros(B * Tq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B * H * Tq + 64, device=dev)
    lib.call(lib.OP_ATTN_FWD, lib.AttnDesc(q=p(q), k=p(k), vt=p(vt), o=p(o), lse=p(lse), B=B, H=H, Tq=Tq, Tk=Tk, ldq=C,
                                           ldk=C, ldvt=ldvt, ldo=C, scale=sc, D=D), stream())
    kt, ldkt = tr(k, Tk)
    qt, ldqt = tr(q, Tq)
    dot, _ = tr(go, Tq)
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    delta = torch.zeros(B * H * Tq + 64, device=dev)
    d = lib.AttnBwdDesc(q=p(q), k=p(k), v=p(v), o=p(o), d_o=p(go), kt=p(kt), qt=p(qt), dot=p(dot), lse=p(lse),
                        delta=p(delta), dq=p(dq), dk=p(dk), dv=p(dv), B=B, H=H, Tq=Tq, Tk=Tk, ldq=C, ldk=C, ldv=C, ldo=C,
                        lddo=C, ldkt=ldkt, ldqt=ldqt, lddq=C, lddk=C, lddv=C, scale=sc, need_dkv=dkv, D=D)
    lib.call(lib.OP_ATTN_BWD, d, stream())
    torch.cuda.synchronize()
    qf = q.float().reshape(B, Tq, H, D).transpose(1, 2).requires_grad_(True)
    kf = k.float().reshape(B, Tk, H, D).transpose(1, 2).requires_grad_(True)
    vf = v.float().reshape(B, Tk, H, D).transpose(1, 2).requires_grad_(True)
    out = torch.softmax(qf @ kf.transpose(-1, -2) * sc, -1) @ vf
    out.backward(go.float().reshape(B, Tq, H, D).transpose(1, 2))
    report(f"attn_bwd dq B{B} H{H} Tq{Tq} Tk{Tk} D{D}", dq, qf.grad.transpose(1, 2).reshape(B * Tq, C), 1.5e-2)
    if dkv:
        report("attn_bwd dk", dk, kf.grad.transpose(1, 2).reshape(B * Tk, C), 1.5e-2)
        report("attn_bwd dv", dv, vf.grad.transpose(1, 2).reshape(B * Tk, C), 1.5e-2)


def test_lora_backward_helpers(dev):
    torch.manual_seed(22)
    M, N, K = 700, 320, 640
    gy = bf(torch.randn(M, N, device=dev))
    up = bf(torch.randn(N, 4, device=dev))
    U = torch.zeros(M, 4, device=dev)
    lib.call(lib.OP_SKINNY, lib.SkinnyDesc(a0=p(gy), w=p(up), out=p(U), lda0=N, ca0=N, mode=0, stride=1, M=M, R=4, K=N,
                                           ldo=4, w_kmajor=1), stream())
    torch.cuda.synchronize()
    report("skinny_kmajor (U = dY.B)", U, gy.float() @ up.float(), 1e-5)
    # dgrad GEMM with the r-major LoRA term: gx = gy.W + s*U12.A12
    wT = bf(torch.randn(K, N, device=dev) / math.sqrt(N))
    U12 = torch.randn(M, 12, device=dev)
    A12 = bf(torch.randn(12, K, device=dev))
    scale = torch.tensor([0.25], device=dev)
    prev = bf(torch.randn(M, K, device=dev))
    gx = prev.clone()
    d = lib.GemmDesc(a0=p(gy), w=p(wT), c=p(gx), residual=p(gx), lora_t=p(U12), lora_up=p(A12), lora_scale=p(scale),
                     lda0=N, ca0=N, mode=0, stride=1, ldw=N, M=M, N=K, K=N, ld_res=K, ldc=K, rows_per_sample=M, ld_t=12,
                     lora_groups=1, lora_rank=12, lora_up_rmajor=1)
    lib.call(lib.OP_GEMM, d, stream())
    torch.cuda.synchronize()
    report("gemm dgrad + rmajor lora + accumulate", gx, gy.float() @ wT.float().t() + 0.25 * U12 @ A12.float() + prev.float(), 6e-3)
    # LoRA conv dgrad, stride 1 and 2
    for stride in (1, 2):
        B, Hl, Wl, Ci = 2, 12, 16, 64
        Ho, Wo = (Hl - 1) // stride + 1, (Wl - 1) // stride + 1
        Uc = torch.randn(B * Ho * Wo, 4, device=dev)
        A4 = bf(torch.randn(4, Ci, 3, 3, device=dev))
        gxi = bf(torch.randn(B * Hl * Wl, Ci, device=dev))
        g0 = gxi.clone()
        a_down = A4.permute(0, 2, 3, 1).reshape(4, -1).contiguous()      # named: alive until the synchronize behind the launch
        dd = lib.LoraCdgradDesc(u=p(Uc), a_down=p(a_down), scale=p(scale),
                                gx=p(gxi), batch=B, hl=Hl, wl=Wl, ho=Ho, wo=Wo, stride=stride, cin=Ci, ldu=4, ldgx=Ci,
                                accumulate=1)
        lib.call(lib.OP_LORA_CONV_DGRAD, dd, stream())
        torch.cuda.synchronize()
        xi = torch.zeros(B, Ci, Hl, Wl, device=dev, requires_grad=True)
        F.conv2d(xi, A4.float(), stride=stride, padding=1).backward(Uc.view(B, Ho, Wo, 4).permute(0, 3, 1, 2))
        ref = g0.float() + 0.25 * xi.grad.permute(0, 2, 3, 1).reshape(B * Hl * Wl, Ci)
        report(f"lora_conv_dgrad stride{stride}", gxi, ref, 6e-3)
    # time_emb_proj adapter gradients
    C, ted = 320, 1280
    g = torch.randn(C, device=dev)
    t = torch.randn(4, device=dev)
    upw = bf(torch.randn(C, 4, device=dev))
    emb = bf(torch.randn(ted, device=dev))
    d_up = torch.zeros(C, 4, device=dev)
    d_dn = torch.zeros(4, ted, device=dev)
    lib.call(lib.OP_TEMB_LORA_BWD, lib.TembLoraBwdDesc(g=p(g), t=p(t), up=p(upw), emb=p(emb), d_up=p(d_up), d_down=p(d_dn),
                                                       scale=p(scale), C=C, ted=ted), stream())
    torch.cuda.synchronize()
    x = bf(F.silu(emb.float())).float()
    report("temb_lora d_up", d_up, 0.25 * g[:, None] * t[None, :], 1e-5)
    report("temb_lora d_down", d_dn, 0.25 * (g @ upw.float())[:, None] * x[None, :], 1e-5)
    # upsample backward + column sums
    B, h, w, Cc = 2, 6, 10, 64
    gu = bf(torch.randn(B * 4 * h * w, Cc, device=dev))
    out = torch.zeros(B * h * w, Cc, device=dev, dtype=torch.bfloat16)
    lib.call(lib.OP_ELEMENTWISE, lib.EwDesc(a=p(gu), out=p(out), M=B * h * w, C=Cc, lda=Cc, ldo=Cc, op=lib.EW_UPSAMPLE_BWD,
                                            iarg=w, iarg2=h * w), stream())
    cs = torch.zeros(B, Cc, device=dev)
    lib.call(lib.OP_ELEMENTWISE, lib.EwDesc(a=p(gu), out=p(cs), M=B * 4 * h * w, C=Cc, lda=Cc, ldo=Cc, op=lib.EW_COLSUM,
                                            iarg2=4 * h * w), stream())
    torch.cuda.synchronize()
    ref = gu.float().view(B, h, 2, w, 2, Cc).sum((2, 4)).reshape(B * h * w, Cc)
    report("upsample_bwd", out, ref, 6e-3)
    report("colsum", cs, gu.float().view(B, -1, Cc).sum(1), 1e-5)


def _oracle_grads(name, method, sd, x, ctx, kw, G, dtype, store):
    net = build_unet(name, seed=0)
    nw = LoRANetworkOracle(net, rank=4, multiplier=1.0, alpha=1.0, train_method=method)
    nw.load_state_dict(sd, strict=True)
    net.to(dtype)
    nw.to(dtype)
    for prm in nw.parameters():
        prm.requires_grad_(True)
    kwd = {k: v.to(dtype) for k, v in kw.items()} if kw else None
    with nw:
        eps = net(x.to(dtype), torch.tensor(600), ctx.to(dtype), kwd).sample
    (eps[1:].float() * G).sum().backward()
    flat = torch.zeros(store.numel)
    mods = {m.lora_name: m for m in nw.unet_loras}
    for e in store.entries:
        m = mods[e.name]
        flat[e.down_off:e.down_off + e.down_numel] = store._down_to_kernel(e, m.lora_down.weight.grad.float())
        flat[e.up_off:e.up_off + e.up_numel] = m.lora_up.weight.grad.float().reshape(-1)
    return flat, eps.detach().float()


@pytest.mark.parametrize("name,method", [("tiny_sdxl", "noxattn"), ("tiny_sd1", "noxattn"), ("tiny_sdxl", "full")])
def test_unet_lora_gradients(dev, name, method):
    cfg = CONFIGS[name]()
    hw = 16
    store = LoraStore(cfg, rank=4, alpha=1.0, train_method=method, device=dev)
    g = torch.Generator().manual_seed(7)
    up_like = (torch.randn(store.numel, generator=g) * 0.05).to(torch.bfloat16)
    for e in store.entries:
        store.params[e.up_off:e.up_off + e.up_numel] = up_like[e.up_off:e.up_off + e.up_numel].to(dev)
    sd = store.state_dict()
    x, ctx, kw = make_inputs(cfg, 2, hw)
    G = torch.randn(1, 4, hw, hw, generator=g)
    G = G.to(torch.bfloat16).float()
    g32, e32 = _oracle_grads(name, method, sd, x, ctx, kw, G, torch.float32, store)
    gbf, _ = _oracle_grads(name, method, sd, x, ctx, kw, G, torch.bfloat16, store)

    eng = UNetEngine(cfg, build_unet(name, seed=0).state_dict(), dev)
    eng.attach_lora(store)
    eng.set_lora(True, 1.0)
    kwd = {k: v.to(dev) for k, v in kw.items()} if kw else None
    out = eng(x.to(dev), torch.tensor(600), ctx.to(dev), kwd, mode="train").sample
    store.grads.zero_()
    eng.run_backward(d_eps=G.to(dev))
    torch.cuda.synchronize()
    got = store.grads.float().cpu()
    r_eng, r_ref = rel_err(got, g32), rel_err(gbf, g32)
    cos = F.cosine_similarity(got, g32, dim=0).item()
    print(f"[parity] lora grads {name} {method}: engine rel_l2={r_eng:.3e} cos={cos:.6f} | torch-bf16 arm rel_l2={r_ref:.3e}"
          f" | |g|={g32.norm():.3e} n={store.numel}")
    # per-kind breakdown helps localise a broken backward op
    worst = []
    for e in store.entries:
        for nm, off, n in (("down", e.down_off, e.down_numel), ("up", e.up_off, e.up_numel)):
            a, b = got[off:off + n], g32[off:off + n]
            if b.norm() > 0:
                worst.append((rel_err(a, b), e.name + "." + nm))
    worst.sort(reverse=True)
    for r, nm in worst[:5]:
        print(f"   worst: {nm} rel_l2={r:.3e}")
    assert torch.isfinite(got).all()
    assert cos >= 0.999, f"gradient direction off: cos={cos}"
    assert r_eng <= r_ref + 1e-3      # measured 2.6e-2 (engine) vs 3.1e-2 (bf16 arm)
