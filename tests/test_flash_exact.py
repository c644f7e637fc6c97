"""The four flash attention kernels (flash.hip: forward, delta, dq, dk/dv)
through ``flash_fwd`` / ``flash_bwd`` against float64 references built from
the stored bf16 inputs, with elementwise bounds that have no free constants
(the form of tests/test_gemm_exact.py and tests/test_conv_exact.py).

Notation: u = 2^-8 is one round-to-nearest bf16 rounding, sc = 1/sqrt(dh),
Sx = sc Q K^T with masked entries -inf, P = softmax(Sx),
A_q = sc max_j (|Q| |K|^T)_qj over the unmasked keys of row q,
eps_q = (dh + 2) 2^-23 A_q the fp32 MFMA error of one score (the (n-1) u
summation bound doubled for MFMA-internal rounding, plus the scale multiply)
and c = (S + 4) 2^-23 the same for a sum over keys. ``__expf`` and
``__logf`` are taken at their derived error: the argument rounding
|x| 2^-24 plus 1 ulp of the result.

Forward. The kernel rounds the numerator p to bf16 for the PV MFMA and sums
the denominator from the unrounded p, so with one bf16 store

    |o   - ref_o|   <= u |ref_o| + (u + 2 eps_q + c) (P |V|)
    |lse - ref_lse| <= eps_q + c + (2 A_q + 16) 2^-23 + 2^-23 |ref_lse|

A score error eps moves every p by a factor e^(+-eps), numerator and
denominator alike (2 eps_q); the bf16 p costs u per term; c covers the fp32
accumulation of either sum. lse = m + log(l): eps_q from the scores, c from
the sum, an exp argument of at most 2 A_q rounded once and 1-ulp results of
exp, log and the two additions ((2 A_q + 16) 2^-23 with room), and the final
rounding of lse itself. lse is an fp32 output and its check is the sharp
one: an extra or missing key of probability above about 1e-5 breaks it,
which the o bound cannot see behind u P|V|.

Backward is a function of its arguments, so the reference takes the kernel's
own o and lse (checked above): P = exp(Sx - lse), delta = rowsum(dO o),
dS = sc P (dO V^T - delta), dQ = dS K, dK = dS^T Q and dV = P^T dO, the last
two per q head. With e_q = eps_q + 2^-23 |lse_q| the error of one exponent,

    mag_dS = sc P (|dO| |V|^T + rowsum|dO o|)
    E_dS   = u |dS| + ((dh + 4) 2^-23 + 2 e_q) mag_dS
    E_P    = (u + 2 e_q) P
    |dq - ref| <= u |ref| + E_dS |K|    + c |dS| |K|
    |dk - ref| <= u |ref| + E_dS^T |Q|  + c |dS|^T |Q|
    |dv - ref| <= u |ref| + E_P^T |dO|  + c P^T |dO|

u |dS| and u P are the bf16 packs feeding the second MFMA, (dh + 4) 2^-23
the two dh-long fp32 dot products (dO V^T and delta) with the subtraction
and multiplies, 2 e_q the recomputed P. delta is internal to flash_bwd and
covered through dq and dk.

A truncating store hides behind u P|V|. The equal-key cases (all rows of k
identical) pin it down: every p is exp(0) = 1 exactly, so the u (P|V|) term
is dropped from the o bound, and at S = 64 non-causal P = 2^-6 is exact in
bf16, so u P is dropped from E_P and dv is checked the same way.

Every case runs on views: q, k, v and dout are [:, :S] slices of parents
with 8 more sequence rows of NaN (a load that ignores kv < S or q < S
poisons the result), o, dq, dk and dv are [:, :S, :, :dh] views of NaN
parents with 8 extra rows and a doubled head stride (every element of the
view must be written, nothing outside it). Geometry the cases are chosen
for: forward and dq use 128 q rows per block (4 waves of 32) and
double-buffered 64-key tiles, so a buffer is reused from three tiles up;
dk/dv uses 128 kv rows per block and 32-row q tiles.

Worst observed error / bound on an MI355X over all cases: o 0.95 (the
equal-key case at S = 200; 0.75 on random keys), lse 0.021, dq 0.79,
dk 0.84, dv 0.83. The hardware ``__expf`` / ``__logf`` stay inside the
derived allowance, so no constant above is measured. The fp32 emulation
below gives the same figures to two digits.

The unmarked CPU test emulates the kernels' arithmetic in fp32 (64-key
tiles, running max, bf16-packed P and dS, bf16 stores) on the same inputs:
honest arithmetic stays within 1.0 of every bound on every case, and a
dropped key, an unmasked key past S, a causal mask off by one, a missing
alpha rescale, an omitted delta, a skipped 32-row q tile in dk/dv and a wrong
kv head each exceed 4x on a case that reaches them. A truncating store errs
by less than 2 u |ref|, so against a bound that contains u |ref| it can
reach 2 and never 4: on the equal-key cases it is required to exceed 1.5
(honest arithmetic: at most 1.0)."""

import functools
import math

import pytest
import torch

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip
    from baton_amd.ops import functional as BF

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
U = 2.0 ** -8
E23 = 2.0 ** -23
PAD = 8


def case(S, h, kvh, dh, causal, B=2, kind="rand", std=1.0, layout="plain"):
    return dict(S=S, h=h, kvh=kvh, dh=dh, causal=causal, B=B, kind=kind,
                std=std, layout=layout)


CASES = {
    # one valid lane, one key
    "s1": case(1, 1, 1, 32, False, B=1),
    "s1_causal": case(1, 1, 1, 32, True, B=1),
    # the second wave holds one row; a single half-empty tile
    "s33_causal": case(33, 2, 2, 32, True),
    # exactly one tile, no tail: std 2
    "s64": case(64, 2, 2, 32, False, std=2.0),
    "s64_causal": case(64, 2, 2, 32, True, std=2.0),
    # half-filled second tile, the non-causal kv < S mask; q/k/v are slices
    # of one packed [B,S,3,h,dh] tensor
    "s96_packed_qkv": case(96, 2, 2, 32, False, layout="qkv"),
    # three tiles (buffer reuse), a one-key tail, a second q block and a
    # second dk/dv block of one row, GQA 2
    "s129_gqa2": case(129, 2, 1, 64, False),
    # per-wave causal tile skip, odd S, GQA with two kv heads; k/v are slices
    # of one packed [B,S,2,kvh,dh] tensor
    "s200_causal_gqa2_packed_kv": case(200, 4, 2, 64, True, layout="kv"),
    # three q blocks and three dk/dv blocks, the last of one row, GQA 3
    "s257_causal_gqa3": case(257, 3, 1, 32, True, B=1),
    # dh = 128 (96 KiB of LDS in dk/dv), S % 32 != 0
    "s130_dh128": case(130, 2, 2, 128, False, B=1),
    "s130_dh128_causal": case(130, 2, 2, 128, True, B=1),
    # rising max: the key rows of tile t are scaled by 1, 2, 4, so alpha
    # rescales hard in every tile; scores reach about +-40
    "s192_rising_max": case(192, 1, 1, 64, False, B=1, kind="rising",
                            std=1.6),
    # equal keys: p = 1 exactly, the store of o (and dv at S = 64) is pinned
    "s64_equal_keys": case(64, 2, 2, 32, False, kind="equal"),
    "s129_gqa2_equal_keys": case(129, 2, 1, 64, False, kind="equal"),
    "s200_causal_gqa2_equal_keys": case(200, 4, 2, 64, True, kind="equal"),
}


def exact_p(c):
    """P = 2^-6 is exact in bf16: u P drops out of E_P."""
    return c["kind"] == "equal" and c["S"] == 64 and not c["causal"]


def kv_map(c):
    g = c["h"] // c["kvh"]
    return [hq // g for hq in range(c["h"])]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Stored bf16 q [B,S,h,dh], k, v [B,S,kvh,dh] and dout [B,S,h,dh];
    different data in every batch and head. Never modified."""
    c = CASES[name]
    B, S, h, kvh, dh = c["B"], c["S"], c["h"], c["kvh"], c["dh"]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(name))
    q = torch.randn(B, S, h, dh, generator=g).mul(c["std"])
    if c["kind"] == "equal":
        k = torch.randn(B, 1, kvh, dh, generator=g).expand(B, S, kvh, dh)
    else:
        k = torch.randn(B, S, kvh, dh, generator=g).mul(c["std"])
    if c["kind"] == "rising":
        k = k * (2.0 ** (torch.arange(S) // 64).double()).float()[None, :, None,
                                                                  None]
    v = torch.randn(B, S, kvh, dh, generator=g).add(0.25)
    dout = torch.randn(B, S, h, dh, generator=g).sub(0.25)
    return tuple(t.to(BF16).contiguous() for t in (q, k, v, dout))


def hf(t):
    """[B,S,h,dh] -> float64 [B,h,S,dh]"""
    return t.double().permute(0, 2, 1, 3)


def keep_mask(c):
    S = c["S"]
    if not c["causal"]:
        return torch.ones(S, S, dtype=torch.bool)
    return torch.ones(S, S, dtype=torch.bool).tril()


def fwd_reference(c, q, k, v):
    """float64 o [B,S,h,dh] and lse [B*h,S] with their bounds."""
    S, dh, B, h = c["S"], c["dh"], c["B"], c["h"]
    sc = 1.0 / math.sqrt(dh)
    kvm = kv_map(c)
    Q, K, V = hf(q), hf(k)[:, kvm], hf(v)[:, kvm]
    keep = keep_mask(c)
    Sx = (sc * Q @ K.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(Sx, dim=-1)
    P = torch.exp(Sx - lse[..., None])
    o = P @ V
    Aq = (sc * Q.abs() @ K.abs().transpose(-1, -2)).masked_fill(
        ~keep, 0.0).amax(dim=-1)
    eps = (dh + 2) * E23 * Aq
    cc = (S + 4) * E23
    up = 0.0 if c["kind"] == "equal" else U
    lim_o = U * o.abs() + (up + 2 * eps + cc)[..., None] * (P @ V.abs())
    lim_lse = eps + cc + (2 * Aq + 16) * E23 + E23 * lse.abs()
    back = lambda t: t.permute(0, 2, 1, 3)
    return dict(o=back(o), lim_o=back(lim_o), lse=lse.reshape(B * h, S),
                lim_lse=lim_lse.reshape(B * h, S))


def bwd_reference(c, q, k, v, dout, o, lse):
    """float64 dq, dk, dv (dk, dv per q head) from the given o and lse, with
    their bounds; everything [B,S,h,dh]."""
    S, dh, B, h = c["S"], c["dh"], c["B"], c["h"]
    sc = 1.0 / math.sqrt(dh)
    kvm = kv_map(c)
    Q, K, V, dO, O = hf(q), hf(k)[:, kvm], hf(v)[:, kvm], hf(dout), hf(o)
    L = lse.double().reshape(B, h, S)
    keep = keep_mask(c)
    T = lambda t: t.transpose(-1, -2)
    Sx = sc * Q @ T(K)
    P = torch.where(keep, torch.exp(Sx - L[..., None]), 0.0)
    Aq = (sc * Q.abs() @ T(K.abs())).masked_fill(~keep, 0.0).amax(dim=-1)
    e = ((dh + 2) * E23 * Aq + E23 * L.abs())[..., None]
    cc = (S + 4) * E23
    delta = (dO * O).sum(-1)[..., None]
    dS = sc * P * (dO @ T(V) - delta)
    mag = sc * P * (dO.abs() @ T(V.abs()) + (dO * O).abs().sum(-1)[..., None])
    E_dS = U * dS.abs() + ((dh + 4) * E23 + 2 * e) * mag
    E_P = ((0.0 if exact_p(c) else U) + 2 * e) * P
    dq, dk, dv = dS @ K, T(dS) @ Q, T(P) @ dO
    lim_dq = U * dq.abs() + E_dS @ K.abs() + cc * dS.abs() @ K.abs()
    lim_dk = U * dk.abs() + T(E_dS) @ Q.abs() + cc * T(dS.abs()) @ Q.abs()
    lim_dv = U * dv.abs() + T(E_P) @ dO.abs() + cc * T(P) @ dO.abs()
    back = lambda t: t.permute(0, 2, 1, 3)
    return dict(dq=back(dq), lim_dq=back(lim_dq), dk=back(dk),
                lim_dk=back(lim_dk), dv=back(dv), lim_dv=back(lim_dv))


def worst(got, ref, lim):
    """max error / bound; anything non-finite, or any error where the bound
    is 0, counts as infinite."""
    got = got.double()
    err = (got - ref).abs()
    r = torch.where(lim > 0, err / lim,
                    torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return r.max().item()


# ---- GPU: the raw ops on padded inputs and strided outputs --------------------

def padded_inputs(c, q, k, v, dout):
    """The case's inputs as [:, :S] views of device parents whose PAD tail
    rows are NaN; layout "qkv" packs q/k/v into one [B,S,3,h,dh] parent,
    "kv" packs k/v into one [B,S,2,kvh,dh] parent."""
    B, S = c["B"], c["S"]

    def parent(*mid):
        return torch.full((B, S + PAD) + mid, float("nan"), dtype=BF16,
                          device=DEV)

    def own(t):
        p = parent(*t.shape[2:])
        p[:, :S] = t.to(DEV)
        return p[:, :S]

    if c["layout"] == "qkv":
        p = parent(3, c["h"], c["dh"])
        for i, t in enumerate((q, k, v)):
            p[:, :S, i] = t.to(DEV)
        qd, kd, vd = p[:, :S, 0], p[:, :S, 1], p[:, :S, 2]
    elif c["layout"] == "kv":
        p = parent(2, c["kvh"], c["dh"])
        p[:, :S, 0], p[:, :S, 1] = k.to(DEV), v.to(DEV)
        qd, kd, vd = own(q), p[:, :S, 0], p[:, :S, 1]
    else:
        qd, kd, vd = own(q), own(k), own(v)
    return qd, kd, vd, own(dout)


def canary_output(c):
    """(parent, view): a NaN [B,S+PAD,h,2dh] parent and its [:, :S, :, :dh]
    view, so the head stride is doubled."""
    parent = torch.full((c["B"], c["S"] + PAD, c["h"], 2 * c["dh"]),
                        float("nan"), dtype=BF16, device=DEV)
    return parent, parent[:, :c["S"], :, :c["dh"]]


def check_canary(tag, c, parent):
    """The view is finite everywhere, the rest of the parent still NaN;
    returns the view on the CPU."""
    p = parent.cpu()
    inside = torch.zeros(p.shape, dtype=torch.bool)
    inside[:, :c["S"], :, :c["dh"]] = True
    assert torch.isfinite(p[inside]).all(), f"{tag}: unwritten or non-finite"
    assert torch.isnan(p[~inside]).all(), f"{tag}: wrote outside its view"
    return p[:, :c["S"], :, :c["dh"]]


def check_route(c, varlen=False, **views):
    """flash_route (csrc/attn_route.h, what flash_fwd / flash_bwd refuse and
    launch from) takes the case with these views (name -> tensor; the others
    contiguous) and names the expected grids, G and LDS sizes."""
    B, S, h, dh = c["B"], c["S"], c["h"], c["dh"]
    d = OPS.flash_route(B, S, h, c["kvh"], dh, causal=c["causal"],
                        varlen=varlen, bwd=True,
                        views={n: [*t.stride(), t.data_ptr() % 16]
                               for n, t in views.items()})
    assert d["eligible"], d["refusal"]
    tiles = (-(-S // 128), B * h)
    assert d["grid_fwd"] == d["grid_dq"] == d["grid_dkv"] == tiles
    assert d["grid_delta"] == (-(-S // 4), B * h)
    assert d["G"] == h // c["kvh"]
    assert (d["lds_fwd"], d["lds_dq"], d["lds_dkv"]) == \
        (512 * dh, 384 * dh, 768 * dh)


@functools.lru_cache(maxsize=None)
def raw_run(name):
    """flash_fwd then flash_bwd on the case's views; CPU copies of o, lse,
    dq, dk, dv after the canary checks."""
    c = CASES[name]
    q, k, v, dout = inputs(name)
    qd, kd, vd, dod = padded_inputs(c, q, k, v, dout)
    assert BF._flash_eligible(qd, kd, vd)
    po, o = canary_output(c)
    outs = [canary_output(c) for _ in range(3)]
    check_route(c, q=qd, k=kd, v=vd, o=o, dout=dod, dq=outs[0][1],
                dk=outs[1][1], dv=outs[2][1])
    ret, lse = OPS.flash_fwd(qd, kd, vd, o, c["causal"])
    assert ret.data_ptr() == o.data_ptr()
    assert lse.dtype == FP32 and tuple(lse.shape) == (c["B"] * c["h"], c["S"])
    OPS.flash_bwd(qd, kd, vd, o, dod, lse, outs[0][1], outs[1][1], outs[2][1],
                  c["causal"])
    res = dict(o=check_canary("o", c, po), lse=lse.cpu())
    for tag, (parent, _) in zip(("dq", "dk", "dv"), outs):
        res[tag] = check_canary(tag, c, parent)
    assert torch.isfinite(res["lse"]).all()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_flash(name):
    c = CASES[name]
    q, k, v, dout = inputs(name)
    got = raw_run(name)
    f = fwd_reference(c, q, k, v)
    b = bwd_reference(c, q, k, v, dout, got["o"], got["lse"])
    ratios = {
        "o": worst(got["o"], f["o"], f["lim_o"]),
        "lse": worst(got["lse"], f["lse"], f["lim_lse"]),
        "dq": worst(got["dq"], b["dq"], b["lim_dq"]),
        "dk": worst(got["dk"], b["dk"], b["lim_dk"]),
        "dv": worst(got["dv"], b["dv"], b["lim_dv"]),
    }
    print(f"flash_exact {name}: worst error / bound = "
          + ", ".join(f"{t} {r:.4f}" for t, r in ratios.items()))
    for t, r in ratios.items():
        assert r <= 1.0, f"{name}: {t} error is {r:.3f} x the bound"


# ---- the wrappers only add plumbing ------------------------------------------

@pytest.mark.gpu
def test_attention_qkv_is_the_raw_ops():
    name = "s96_packed_qkv"
    c = CASES[name]
    q, k, v, dout = inputs(name)
    raw = raw_run(name)
    qkv = torch.stack((q, k, v), dim=2).to(DEV).requires_grad_(True)
    assert BF._flash_eligible(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    o = BF.attention_qkv(qkv, c["causal"])
    o.backward(dout.to(DEV))
    assert torch.equal(o.detach().cpu(), raw["o"])
    for i, tag in enumerate(("dq", "dk", "dv")):
        assert torch.equal(qkv.grad[:, :, i].cpu(), raw[tag]), tag


@pytest.mark.gpu
def test_attention_bshd_gqa_group_sum():
    name = "s200_causal_gqa2_packed_kv"
    c = CASES[name]
    B, S, h, kvh, dh = c["B"], c["S"], c["h"], c["kvh"], c["dh"]
    g = h // kvh
    q, k, v, dout = inputs(name)
    raw = raw_run(name)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    assert BF._flash_eligible(qd, kd, vd)
    o = BF.attention_bshd(qd, kd, vd, c["causal"])
    o.backward(dout.to(DEV))
    assert torch.equal(o.detach().cpu(), raw["o"])
    assert torch.equal(qd.grad.cpu(), raw["dq"])
    # kv head j serves q heads j g .. j g + g - 1: one fp32 sum of g stored
    # bf16 terms and one bf16 store
    for tag, grad in (("dk", kd.grad), ("dv", vd.grad)):
        terms = raw[tag].double().view(B, S, kvh, g, dh)
        ref = terms.sum(3)
        lim = U * ref.abs() + g * E23 * terms.abs().sum(3)
        r = worst(grad.cpu(), ref, lim)
        print(f"flash_exact bshd {tag} group sum: worst error / bound = "
              f"{r:.4f}")
        assert r <= 1.0, f"{tag}: {r:.3f} x the bound"


@pytest.mark.gpu
def test_flash_gate(monkeypatch):
    monkeypatch.delenv("BATON_NO_FLASH", raising=False)

    def eligible(q, k, v, refusal=None):
        """_flash_eligible, which is false exactly when flash_fwd refuses
        the views, with flash_route's text ``refusal`` (both are its
        answer)."""
        e = BF._flash_eligible(q, k, v)
        assert e == (refusal is None)
        o = torch.empty(q.shape, dtype=BF16, device=DEV)
        if e:
            OPS.flash_fwd(q, k, v, o, False)
        else:
            with pytest.raises(RuntimeError, match=refusal):
                OPS.flash_fwd(q, k, v, o, False)
        return e

    ok = torch.zeros(1, 32, 2, 32, dtype=BF16, device=DEV)
    assert eligible(ok, ok, ok)
    f32 = torch.randn(1, 32, 2, 32, device=DEV)
    assert not eligible(f32, f32, f32, "q must be a bf16 GPU tensor")
    dh48 = torch.zeros(1, 32, 2, 48, dtype=BF16, device=DEV)
    assert not eligible(dh48, dh48, dh48, "unsupported head_dim 48")
    # misaligned views take the legacy path instead of raising: a base
    # pointer 8 bytes in, and a head stride of dh + 4
    off = torch.zeros(1 * 32 * 2 * 32 + 4, dtype=BF16, device=DEV)[4:].view(
        1, 32, 2, 32)
    assert not eligible(off, ok, ok, "q must start on a 16-byte boundary")
    assert not eligible(ok, off, ok, "k must start on a 16-byte boundary")
    odd = torch.zeros(1, 32, 2, 36, dtype=BF16, device=DEV)[..., :32]
    assert not eligible(ok, ok, odd, "v strides must be multiples of 8")
    monkeypatch.setenv("BATON_NO_FLASH", "1")
    assert not BF._flash_eligible(ok, ok, ok)
    monkeypatch.delenv("BATON_NO_FLASH")
    assert BF._flash_eligible(ok, ok, ok)
    out = BF.attention_bshd(f32, f32, f32, True)
    assert out.dtype == FP32 and tuple(out.shape) == (1, 32, 2, 32)
    assert torch.isfinite(out).all()


# ---- refused on the host, before any allocation or launch ----------------------

SENTINEL = 7.0


def _valid(B=2, S=64, h=4, kvh=2, dh=64):
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    s = lambda *s_: torch.full(s_, SENTINEL, dtype=BF16, device=DEV)
    return dict(q=z(B, S, h, dh), k=z(B, S, kvh, dh), v=z(B, S, kvh, dh),
                o=s(B, S, h, dh), dout=z(B, S, h, dh),
                lse=torch.zeros(B * h, S, device=DEV),
                dq=s(B, S, h, dh), dk=s(B, S, h, dh), dv=s(B, S, h, dh))


def _misaligned(t):
    """The same sizes, 8 bytes off a 16-byte boundary."""
    flat = torch.full((t.numel() + 4,), SENTINEL, dtype=BF16, device=DEV)
    return flat[4:].view(t.shape)


def _odd_stride(t, dim):
    """The same sizes, all SENTINEL, with stride(dim) alone 4 elements over
    the contiguous one (S = 64 keeps the batch stride a multiple of 8 when
    the sequence stride is not)."""
    st = list(t.contiguous().stride())
    st[dim] += 4
    if dim == 1:
        st[0] = t.shape[1] * st[1]
    room = 1 + sum((n - 1) * s for n, s in zip(t.shape, st))
    flat = torch.full((room,), SENTINEL, dtype=BF16, device=DEV)
    return flat.as_strided(tuple(t.shape), tuple(st))


SHARE = "share q's B, S and dh"
VIEW = "bf16 GPU tensor"
ALIGN = "16-byte boundary"
STRIDE = "multiples of 8"
SIZES = "must have q's sizes"


def _bad_inputs(args):
    """name -> (argument, replacement, message) for every tensor in
    ``args``: what both ops refuse in any of their views, and what they
    refuse in k and v."""
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    ok = _valid()
    bad = {
        "k_seq": ("k", z(2, 32, 2, 64), SHARE),
        "k_batch": ("k", z(1, 64, 2, 64), SHARE),
        "k_head_dim": ("k", z(2, 64, 2, 32), SHARE),
        "v_seq": ("v", z(2, 72, 2, 64)[:, :63], SHARE),
        "v_batch": ("v", z(3, 64, 2, 64), SHARE),
        "v_head_dim": ("v", z(2, 64, 2, 128), SHARE),
        "kv_head_counts_differ": ("v", z(2, 64, 4, 64), "same head count"),
        "k_cpu": ("k", torch.zeros(2, 64, 2, 64, dtype=BF16), VIEW),
        "q_fp32": ("q", torch.zeros(2, 64, 4, 64, device=DEV), VIEW),
        "q_rank": ("q", z(2, 64, 256), "must be .B,S,h,dh."),
        "v_head_dim_strided": ("v", z(2, 64, 2, 128)[..., ::2],
                               "head_dim must be contiguous"),
    }
    for arg in args:
        bad[f"{arg}_misaligned"] = (arg, _misaligned(ok[arg]), ALIGN)
        for dim in range(3):
            bad[f"{arg}_stride{dim}"] = (arg, _odd_stride(ok[arg], dim),
                                         STRIDE)
    return bad


def _full(*shape):
    return torch.full(shape, SENTINEL, dtype=BF16, device=DEV)


@pytest.mark.gpu
def test_flash_fwd_refuses():
    bad = _bad_inputs(("q", "k", "v", "o"))
    bad.update({
        "o_seq": ("o", _full(2, 72, 4, 64), SIZES),
        "o_heads": ("o", _full(2, 64, 2, 64), SIZES),
        "o_batch": ("o", _full(1, 64, 4, 64), SIZES),
        "o_head_dim": ("o", _full(2, 64, 4, 128), SIZES),
        # 3 q heads over 2 kv heads; dh = 48 has no kernel
        "heads_not_a_multiple": (None, dict(h=3), "multiple of kv heads"),
        "head_dim_48": (None, dict(dh=48), "unsupported head_dim"),
    })
    for what, (arg, repl, msg) in bad.items():
        a = _valid(**repl) if arg is None else _valid()
        if arg is not None:
            a[arg] = repl
        with pytest.raises(RuntimeError, match=msg):
            OPS.flash_fwd(a["q"], a["k"], a["v"], a["o"], False)
        torch.cuda.synchronize()
        assert (a["o"].float() == SENTINEL).all(), what
        print(f"flash_exact flash_fwd refused {what}")
    a = _valid()
    OPS.flash_fwd(a["q"], a["k"], a["v"], a["o"], False)
    assert (a["o"] == 0).all()


@pytest.mark.gpu
def test_flash_bwd_refuses():
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    bad = _bad_inputs(("q", "k", "v", "o", "dout", "dq", "dk", "dv"))
    LSE = "lse must be"
    bad.update({
        "heads_not_a_multiple": (None, dict(h=3), "multiple of kv heads"),
        "head_dim_48": (None, dict(dh=48), "unsupported head_dim"),
        "o_seq": ("o", z(2, 72, 4, 64), SIZES),
        "dout_heads": ("dout", z(2, 64, 2, 64), SIZES),
        "dout_batch": ("dout", z(1, 64, 4, 64), SIZES),
        "dq_seq": ("dq", _full(2, 72, 4, 64), SIZES),
        "dq_head_dim": ("dq", _full(2, 64, 4, 32), SIZES),
        "dk_kv_heads": ("dk", _full(2, 64, 2, 64), SIZES),
        "dv_kv_heads": ("dv", _full(2, 64, 2, 64), SIZES),
        "dk_seq": ("dk", _full(2, 65, 4, 64), SIZES),
        "dv_seq": ("dv", _full(2, 63, 4, 64), SIZES),
        "lse_seq": ("lse", torch.zeros(8, 65, device=DEV), LSE),
        "lse_rows": ("lse", torch.zeros(4, 64, device=DEV), LSE),
        "lse_rank": ("lse", torch.zeros(2, 4, 64, device=DEV), LSE),
        "lse_transposed": ("lse", torch.zeros(64, 8, device=DEV).t(), LSE),
        "lse_bf16": ("lse", z(8, 64), LSE),
        "lse_cpu": ("lse", torch.zeros(8, 64), LSE),
    })
    for what, (arg, repl, msg) in bad.items():
        a = _valid(**repl) if arg is None else _valid()
        if arg is not None:
            a[arg] = repl
        with pytest.raises(RuntimeError, match=msg):
            OPS.flash_bwd(a["q"], a["k"], a["v"], a["o"], a["dout"], a["lse"],
                          a["dq"], a["dk"], a["dv"], False)
        torch.cuda.synchronize()
        for out in ("dq", "dk", "dv"):
            assert (a[out].float() == SENTINEL).all(), (what, out)
        print(f"flash_exact flash_bwd refused {what}")
    a = _valid()
    a["o"].zero_()
    OPS.flash_bwd(a["q"], a["k"], a["v"], a["o"], a["dout"], a["lse"],
                  a["dq"], a["dk"], a["dv"], False)
    for out in ("dq", "dk", "dv"):
        assert (a[out] == 0).all(), out


# ---- CPU: the bounds admit honest fp32 and reject single defects ---------------

def rbf(t, truncate=False):
    """fp32 -> bf16 -> fp32, round to nearest even or truncating."""
    if truncate:
        return (t.contiguous().view(torch.int32) & -65536).view(FP32)
    return t.to(BF16).float()


def _f(t):
    """[B,S,h,dh] -> fp32 [B,h,S,dh]"""
    return t.float().permute(0, 2, 1, 3).contiguous()


def _tile(t, lo, n):
    """rows lo .. lo+n-1 of [B,h,S,dh], zero rows past S (the guarded loads)"""
    S = t.shape[2]
    out = t.new_zeros(t.shape[:2] + (n, t.shape[3]))
    hi = min(S, lo + n)
    if hi > lo:
        out[:, :, :hi - lo] = t[:, :, lo:hi]
    return out


def emulate_fwd(c, q, k, v, mutant=None):
    """flash_fwd_kernel in fp32: 64-key tiles, running max and sum, p rounded
    to bf16 for the PV product only, one bf16 store of o; lse = m + log l."""
    S, dh = c["S"], c["dh"]
    sc = 1.0 / math.sqrt(dh)
    kvm = kv_map(c)
    if mutant == "wrong_kv_head":
        kvm = [hq % c["kvh"] for hq in range(c["h"])]
    Q, K, V = _f(q), _f(k)[:, kvm], _f(v)[:, kvm]
    qi = torch.arange(S)[:, None]
    m = Q.new_full(Q.shape[:3], float("-inf"))
    l = Q.new_zeros(Q.shape[:3])
    acc = torch.zeros_like(Q)
    for k0 in range(0, S, 64):
        kv = torch.arange(k0, k0 + 64)[None, :]
        valid = kv < (S + 1 if mutant == "unmasked_key_past_S" else S)
        if c["causal"]:
            valid = valid & (kv <= qi + (mutant == "causal_off_by_one"))
        else:
            valid = valid.expand(S, 64)
        if mutant == "dropped_key":
            valid = valid & (kv != S // 2)
        Kt, Vt = _tile(K, k0, 64), _tile(V, k0, 64)
        s = (Q @ Kt.transpose(-1, -2)) * sc
        s = torch.where(valid, s, torch.full_like(s, -1e30))
        mn = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.exp(m - mn)
        m = mn
        p = torch.exp(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        if mutant != "missing_alpha":
            acc = acc * alpha[..., None]
        acc = acc + rbf(p) @ Vt
    o = rbf(acc * (1.0 / l)[..., None], truncate=mutant == "truncating_store")
    lse = m + torch.log(l)
    return (o.permute(0, 2, 1, 3).to(BF16),
            lse.reshape(c["B"] * c["h"], S))


def emulate_bwd(c, q, k, v, dout, o, lse, mutant=None):
    """flash_delta_kernel, flash_bwd_dq_kernel (64-key tiles) and
    flash_bwd_dkv_kernel (32-row q tiles) in fp32: P from lse, dS and P
    rounded to bf16 for the second product, bf16 stores."""
    S, dh = c["S"], c["dh"]
    sc = 1.0 / math.sqrt(dh)
    kvm = kv_map(c)
    if mutant == "wrong_kv_head":
        kvm = [hq % c["kvh"] for hq in range(c["h"])]
    Q, K, V, dO, O = _f(q), _f(k)[:, kvm], _f(v)[:, kvm], _f(dout), _f(o)
    L = lse.float().reshape(Q.shape[:3])[..., None]
    delta = (dO * O).sum(-1)[..., None]
    if mutant == "delta_omitted":
        delta = torch.zeros_like(delta)
    keep = keep_mask(c)
    T = lambda t: t.transpose(-1, -2)
    trunc = mutant == "truncating_store"

    def p_ds(Qr, dOr, Lr, dr, Kc, Vc, kp):
        p = torch.where(kp, torch.exp((Qr @ T(Kc)) * sc - Lr),
                        torch.zeros(()))
        return p, p * (dOr @ T(Vc) - dr) * sc

    dq = torch.zeros_like(Q)
    for k0 in range(0, S, 64):
        k1 = min(S, k0 + 64)
        _, ds = p_ds(Q, dO, L, delta, K[:, :, k0:k1], V[:, :, k0:k1],
                     keep[:, k0:k1])
        dq = dq + rbf(ds) @ K[:, :, k0:k1]
    dk, dv = torch.zeros_like(Q), torch.zeros_like(Q)
    for qt, q0 in enumerate(range(0, S, 32)):
        if mutant == "skipped_q_tile" and qt == 1:
            continue
        q1 = min(S, q0 + 32)
        r = slice(q0, q1)
        p, ds = p_ds(Q[:, :, r], dO[:, :, r], L[:, :, r], delta[:, :, r], K, V,
                     keep[r])
        dv = dv + T(rbf(p)) @ dO[:, :, r]
        dk = dk + T(rbf(ds)) @ Q[:, :, r]
    return tuple(rbf(t, trunc).permute(0, 2, 1, 3).to(BF16)
                 for t in (dq, dk, dv))


def emulated_ratios(name, mutant=None):
    """error / bound of the emulation for o, lse, dq, dk, dv. Forward
    mutants are checked on the forward outputs; the backward always runs on
    an honest forward, as flash_bwd is checked given o and lse."""
    c = CASES[name]
    q, k, v, dout = inputs(name)
    f = fwd_reference(c, q, k, v)
    o, lse = emulate_fwd(c, q, k, v, mutant)
    r = {"o": worst(o, f["o"], f["lim_o"]),
         "lse": worst(lse, f["lse"], f["lim_lse"])}
    if mutant in FWD_ONLY:
        return r
    if mutant is not None:
        o, lse = emulate_fwd(c, q, k, v)
    b = bwd_reference(c, q, k, v, dout, o, lse)
    for tag, got in zip(("dq", "dk", "dv"),
                        emulate_bwd(c, q, k, v, dout, o, lse, mutant)):
        r[tag] = worst(got, b[tag], b["lim_" + tag])
    return r


FWD_ONLY = ("dropped_key", "unmasked_key_past_S", "causal_off_by_one",
            "missing_alpha")
# mutant -> the cases that reach it and the outputs it is judged on
MUTANTS = {
    "dropped_key": ([n for n in CASES if CASES[n]["S"] > 1], ("o", "lse")),
    "unmasked_key_past_S": (
        [n for n in CASES if CASES[n]["S"] % 64 and not CASES[n]["causal"]],
        ("lse",)),
    "causal_off_by_one": (
        [n for n in CASES if CASES[n]["causal"] and CASES[n]["S"] > 1],
        ("o", "lse")),
    "missing_alpha": ([n for n in CASES if CASES[n]["S"] > 64], ("o",)),
    "delta_omitted": (list(CASES), ("dq", "dk")),
    "skipped_q_tile": ([n for n in CASES if CASES[n]["S"] > 32],
                       ("dk", "dv")),
    "wrong_kv_head": ([n for n in CASES if CASES[n]["kvh"] > 1
                       and CASES[n]["h"] > CASES[n]["kvh"]],
                      ("o", "lse", "dq", "dk", "dv")),
}


def test_bounds_admit_fp32_emulation():
    top = {}
    for name in CASES:
        r = emulated_ratios(name)
        print(f"flash_exact emulated {name}: "
              + ", ".join(f"{t} {x:.3f}" for t, x in r.items()))
        for t, x in r.items():
            assert x <= 1.0, f"{name}: honest fp32 {t} is {x:.3f} x the bound"
            top[t] = max(top.get(t, 0.0), x)
    print(f"flash_exact emulated worst: {top}")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bounds_reject(mutant):
    names, outputs = MUTANTS[mutant]
    assert names
    best = 0.0
    for name in names:
        r = emulated_ratios(name, mutant)
        best = max(best, max(r[t] for t in outputs))
    print(f"flash_exact mutant {mutant}: {best:.1f} x the bound")
    assert best > 4.0, f"{mutant} reaches only {best:.2f} x the bound"


def test_bounds_reject_truncating_store():
    """Judged on the outputs whose u P term is dropped: o on every equal-key
    case, dv where P is exact."""
    for name in CASES:
        c = CASES[name]
        if c["kind"] != "equal":
            continue
        honest = emulated_ratios(name)
        r = emulated_ratios(name, "truncating_store")
        print(f"flash_exact truncating store {name}: o {honest['o']:.3f} -> "
              f"{r['o']:.3f}, dv {honest['dv']:.3f} -> {r['dv']:.3f}")
        assert honest["o"] <= 1.0 < 1.5 < r["o"], (name, honest["o"], r["o"])
        if exact_p(c):
            assert honest["dv"] <= 1.0 < 1.5 < r["dv"], (name, r["dv"])
