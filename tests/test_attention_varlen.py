"""Per-sequence lengths (right-padded batches) in flash attention: the
length-aware instantiations of the four flash kernels through ``flash_fwd`` /
``flash_bwd`` with ``seq_lens``, the wrappers ``attention_qkv`` /
``attention_bshd``, and the fp32 emulation of those kernels with the single
defects the checks must catch. The materialized-scores path, the model and
the data helpers are in tests/test_attention_varlen_paths.py.

The contract, for batch element b with length L_b: key j is visible to query
i iff j < L_b (and j <= i if causal); rows < L_b of o, lse, dq, dk, dv are
what the dense op gives on the [b:b+1, :L_b] slices; rows >= L_b are +0.0.

The length-aware kernels are the dense kernels with L_b in place of S: the
same 64-key tiles in the same order under the same mask. So on the GPU the
live rows are required to be *bit-identical* to the dense ``flash_fwd`` /
``flash_bwd`` run on the slices, and they are also held to the float64 bounds
of tests/test_flash_exact.py evaluated for a case with S = L_b, B = 1
(notation and derivation there; nothing here is fitted). Every padded
element must be +0.0 bit for bit: its bound is 0. Worst observed error /
bound on an MI355X over all cases: o 0.83 (equal keys), lse 0.022, dq 0.72,
dk 0.79, dv 0.87; the fp32 emulation below gives the same to two digits.

Inputs as in test_flash_exact.py (views of NaN-padded parents, canaried
strided outputs), and in addition rows >= L_b of q, k, v and dout are NaN:
nothing there may influence any output. Geometry the cases target: 128-row q
blocks of four 32-row waves, 64-key double-buffered tiles, 128-row kv blocks
and 32-row q tiles in dk/dv.

The unmarked CPU tests emulate the length-aware kernels in fp32 (finite
padding, so that a defect gives a figure instead of NaN): honest arithmetic
stays within 1.0 of every bound and reproduces the dense emulation on the
slices bit for bit; the key at j = L_b left visible, the length of batch
b + 1 used for batch b, a dead query row that attends instead of storing
zero, the key loop bound rounded down to whole tiles and dk/dv accumulating
q rows >= L_b each exceed 4x on a case that reaches them."""

import functools
import math

import pytest
import torch

import test_flash_exact as FE
from baton_amd.ops import functional as BF

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = FE.DEV
BF16, FP32 = FE.BF16, FE.FP32
NAN = float("nan")


def vcase(lens, S, h, kvh, dh, causal, **kw):
    c = FE.case(S, h, kvh, dh, causal, B=len(lens), **kw)
    c["lens"] = tuple(lens)
    return c


CASES = {
    # 200: a full row; 129: a one-key third tile and a one-row second block;
    # 64: exactly one tile and a dead second block; 1: a single key
    "s200": vcase((200, 129, 64, 1), 200, 2, 1, 64, False),
    # 130: two rows into the second block; 33: one row in the second wave;
    # 0: an empty sequence
    "s200_causal": vcase((200, 130, 33, 0), 200, 2, 1, 64, True),
    # 128: a length on a block boundary, 127: one short of it; GQA 3
    "s257_causal_gqa3": vcase((257, 128, 127), 257, 3, 1, 32, True),
    # dh = 128
    "s130_dh128": vcase((130, 97), 130, 2, 2, 128, False),
    "s130_dh128_causal": vcase((130, 97), 130, 2, 2, 128, True),
    # q, k, v are slices of one packed [B,S,3,h,dh] tensor
    "s96_packed_qkv": vcase((96, 65, 31), 96, 2, 2, 32, False, layout="qkv"),
    # equal keys: p = 1 exactly, the store rounding of o is pinned (and of
    # dv at L = 64, where P = 2^-6 is exact)
    "s129_equal_keys": vcase((129, 64), 129, 2, 1, 64, False, kind="equal"),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Stored bf16 q, k, v, dout [B,S,*,dh] with finite random data in every
    row, the padded ones included. Never modified."""
    c = CASES[name]
    B, S, h, kvh, dh = c["B"], c["S"], c["h"], c["kvh"], c["dh"]
    g = torch.Generator().manual_seed(9000 + list(CASES).index(name))
    q = torch.randn(B, S, h, dh, generator=g).mul(c["std"])
    if c["kind"] == "equal":
        k = torch.randn(B, 1, kvh, dh, generator=g).expand(B, S, kvh, dh)
    else:
        k = torch.randn(B, S, kvh, dh, generator=g).mul(c["std"])
    v = torch.randn(B, S, kvh, dh, generator=g).add(0.25)
    dout = torch.randn(B, S, h, dh, generator=g).sub(0.25)
    return tuple(t.to(BF16).contiguous() for t in (q, k, v, dout))


def nan_padded(c, *tensors):
    """Copies with rows >= L_b of batch element b set to NaN."""
    out = []
    for t in tensors:
        t = t.clone()
        for b, L in enumerate(c["lens"]):
            t[b, L:] = NAN
        out.append(t)
    return out


def slice_case(c, L):
    """The dense case that batch element b is required to reproduce."""
    cb = dict(c, S=L, B=1)
    cb.pop("lens")
    return cb


@functools.lru_cache(maxsize=None)
def references(name):
    """Per batch element: None for L_b = 0, else the float64 forward
    reference of the [b:b+1, :L_b] slices (the backward reference needs the
    o and lse under test)."""
    c = CASES[name]
    q, k, v, _ = inputs(name)
    refs = []
    for b, L in enumerate(c["lens"]):
        if L == 0:
            refs.append(None)
            continue
        refs.append(FE.fwd_reference(slice_case(c, L), q[b:b + 1, :L],
                                     k[b:b + 1, :L], v[b:b + 1, :L]))
    return refs


def plus_zero(t):
    """Every element is +0.0 bit for bit."""
    if t.numel() == 0:
        return True
    bits = t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)
    return bool((bits == 0).all())


def ratios(name, got):
    """Worst error / bound of got = dict(o, lse, dq, dk, dv) (CPU tensors,
    lse [B*h, S]) over the batch: live rows against the float64 references
    of the slices, padded rows against a bound of 0 (anything but +0.0 is
    infinite)."""
    c = CASES[name]
    q, k, v, dout = inputs(name)
    B, S, h = c["B"], c["S"], c["h"]
    lse = got["lse"].reshape(B, h, S)
    top = {t: 0.0 for t in ("o", "lse", "dq", "dk", "dv")}
    for b, L in enumerate(c["lens"]):
        for t in ("o", "dq", "dk", "dv"):
            if not plus_zero(got[t][b, L:]):
                top[t] = float("inf")
        if not plus_zero(lse[b, :, L:]):
            top["lse"] = float("inf")
        if L == 0:
            continue
        cb = slice_case(c, L)
        f = references(name)[b]
        ob, lb = got["o"][b:b + 1, :L], lse[b, :, :L].contiguous()
        bw = FE.bwd_reference(cb, q[b:b + 1, :L], k[b:b + 1, :L],
                              v[b:b + 1, :L], dout[b:b + 1, :L], ob, lb)
        top["o"] = max(top["o"], FE.worst(ob, f["o"], f["lim_o"]))
        top["lse"] = max(top["lse"], FE.worst(lb, f["lse"], f["lim_lse"]))
        for t in ("dq", "dk", "dv"):
            top[t] = max(top[t], FE.worst(got[t][b:b + 1, :L], bw[t],
                                          bw["lim_" + t]))
    return top


# ---- GPU: the raw ops ----------------------------------------------------------

def lens_tensor(c):
    return torch.tensor(c["lens"], dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def raw_run(name):
    """flash_fwd / flash_bwd with seq_lens on NaN-padded views; CPU copies of
    o, lse, dq, dk, dv after the canary checks (every element of every view
    written and finite, nothing outside it touched)."""
    c = CASES[name]
    q, k, v, dout = nan_padded(c, *inputs(name))
    qd, kd, vd, dod = FE.padded_inputs(c, q, k, v, dout)
    assert BF._flash_eligible(qd, kd, vd)
    lens = lens_tensor(c)
    po, o = FE.canary_output(c)
    outs = [FE.canary_output(c) for _ in range(3)]
    FE.check_route(c, varlen=True, q=qd, k=kd, v=vd, o=o, dout=dod,
                   dq=outs[0][1], dk=outs[1][1], dv=outs[2][1])
    ret, lse = OPS.flash_fwd(qd, kd, vd, o, c["causal"], lens)
    assert ret.data_ptr() == o.data_ptr()
    assert lse.dtype == FP32 and tuple(lse.shape) == (c["B"] * c["h"], c["S"])
    OPS.flash_bwd(qd, kd, vd, o, dod, lse, outs[0][1], outs[1][1], outs[2][1],
                  c["causal"], lens)
    res = dict(o=FE.check_canary("o", c, po), lse=lse.cpu())
    for tag, (parent, _) in zip(("dq", "dk", "dv"), outs):
        res[tag] = FE.check_canary(tag, c, parent)
    assert torch.isfinite(res["lse"]).all()
    assert torch.equal(lens.cpu(), torch.tensor(c["lens"], dtype=torch.int32))
    res["views"] = (qd, kd, vd, dod)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_flash_varlen(name):
    c = CASES[name]
    got = raw_run(name)
    qd, kd, vd, dod = got["views"]
    B, S, h = c["B"], c["S"], c["h"]
    lse = got["lse"].reshape(B, h, S)
    # 1. the live rows are the dense kernels on the slices, bit for bit
    for b, L in enumerate(c["lens"]):
        if L == 0:
            continue
        cb = slice_case(c, L)
        sl = lambda t: t[b:b + 1, :L]
        po, o = FE.canary_output(cb)
        _, lse_b = OPS.flash_fwd(sl(qd), sl(kd), sl(vd), o, c["causal"])
        outs = [FE.canary_output(cb) for _ in range(3)]
        OPS.flash_bwd(sl(qd), sl(kd), sl(vd), o, sl(dod), lse_b, outs[0][1],
                      outs[1][1], outs[2][1], c["causal"])
        dense = dict(o=FE.check_canary("o", cb, po))
        for tag, (parent, _) in zip(("dq", "dk", "dv"), outs):
            dense[tag] = FE.check_canary(tag, cb, parent)
        for tag in ("o", "dq", "dk", "dv"):
            assert torch.equal(got[tag][b:b + 1, :L], dense[tag]), \
                f"{name} b={b} L={L}: {tag} differs from the dense kernel"
        assert torch.equal(lse[b, :, :L], lse_b.cpu()), \
            f"{name} b={b} L={L}: lse differs from the dense kernel"
    # 2. and 3. the float64 bounds on the live rows, +0.0 on the padded ones
    r = ratios(name, got)
    print(f"varlen {name}: worst error / bound = "
          + ", ".join(f"{t} {x:.4f}" for t, x in r.items()))
    for t, x in r.items():
        assert x <= 1.0, f"{name}: {t} error is {x:.3f} x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_seq_lens_none_is_the_plain_call(name):
    c = CASES[name]
    qd, kd, vd, dod = (t.to(DEV) for t in inputs(name))
    res = []
    for extra in ((), (None,)):
        o = torch.empty_like(qd)
        _, lse = OPS.flash_fwd(qd, kd, vd, o, c["causal"], *extra)
        dq, dk, dv = (torch.empty_like(qd) for _ in range(3))
        OPS.flash_bwd(qd, kd, vd, o, dod, lse, dq, dk, dv, c["causal"], *extra)
        res.append((o, lse, dq, dk, dv))
    for tag, a, b in zip(("o", "lse", "dq", "dk", "dv"), *res):
        assert torch.equal(a, b), tag


# ---- GPU: the wrappers only add plumbing -----------------------------------------

@pytest.mark.gpu
def test_attention_qkv_varlen_is_the_raw_ops():
    name = "s96_packed_qkv"
    c = CASES[name]
    raw = raw_run(name)
    q, k, v, dout = nan_padded(c, *inputs(name))
    qkv = torch.stack((q, k, v), dim=2).to(DEV).requires_grad_(True)
    assert BF._flash_eligible(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    lens = lens_tensor(c)
    o = BF.attention_qkv(qkv, c["causal"], seq_lens=lens)
    o.backward(dout.to(DEV))
    assert torch.equal(o.detach().cpu(), raw["o"])
    for i, tag in enumerate(("dq", "dk", "dv")):
        assert torch.equal(qkv.grad[:, :, i].cpu(), raw[tag]), tag
    assert not lens.requires_grad and lens.grad is None
    assert o.grad_fn.next_functions[-1][0] is None    # no edge to seq_lens
    # seq_lens=None is the plain wrapper call
    q, k, v, dout = inputs(name)
    grads = []
    for kw in ({}, {"seq_lens": None}):
        x = torch.stack((q, k, v), dim=2).to(DEV).requires_grad_(True)
        y = BF.attention_qkv(x, c["causal"], **kw)
        y.backward(dout.to(DEV))
        grads.append((y.detach(), x.grad))
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s200", "s200_causal"])
def test_attention_bshd_varlen_gqa_group_sum(name):
    c = CASES[name]
    B, S, h, kvh, dh = c["B"], c["S"], c["h"], c["kvh"], c["dh"]
    g = h // kvh
    assert g == 2     # a two-term fp32 sum is exact in any order
    raw = raw_run(name)
    q, k, v, dout = nan_padded(c, *inputs(name))
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    lens = lens_tensor(c)
    o = BF.attention_bshd(qd, kd, vd, c["causal"], seq_lens=lens)
    o.backward(dout.to(DEV))
    assert torch.equal(o.detach().cpu(), raw["o"])
    assert torch.equal(qd.grad.cpu(), raw["dq"])
    for tag, grad in (("dk", kd.grad), ("dv", vd.grad)):
        want = raw[tag].view(B, S, kvh, g, dh).sum(3, dtype=FP32).to(BF16)
        assert torch.equal(grad.cpu(), want), tag
        for b, L in enumerate(c["lens"]):
            assert plus_zero(grad[b, L:].cpu()), (tag, b)
    assert not lens.requires_grad and lens.grad is None
    assert o.grad_fn.next_functions[-1][0] is None


# ---- GPU: refused on the host, before any allocation or launch -------------------

@pytest.mark.gpu
def test_flash_refuses_bad_seq_lens():
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=DEV)
    bad = {
        "int64": (torch.tensor([64, 64], device=DEV), "seq_lens must be int32"),
        "float": (torch.tensor([64.0, 64.0], device=DEV),
                  "seq_lens must be int32"),
        "strided": (i32(64, 0, 64, 0)[::2], "seq_lens must be contiguous"),
        "cpu": (torch.tensor([64, 64], dtype=torch.int32),
                "seq_lens must be on"),
        "one_short": (i32(64), "seq_lens must have exactly B = 2"),
        "one_over": (i32(64, 64, 64), "seq_lens must have exactly B = 2"),
        "per_head": (i32(*([64] * 8)), "seq_lens must have exactly B = 2"),
    }
    for what, (lens, msg) in bad.items():
        a = FE._valid()
        with pytest.raises(RuntimeError, match=msg):
            OPS.flash_fwd(a["q"], a["k"], a["v"], a["o"], False, lens)
        with pytest.raises(RuntimeError, match=msg):
            OPS.flash_bwd(a["q"], a["k"], a["v"], a["o"], a["dout"], a["lse"],
                          a["dq"], a["dk"], a["dv"], False, lens)
        torch.cuda.synchronize()
        for out in ("o", "dq", "dk", "dv"):
            assert (a[out].float() == FE.SENTINEL).all(), (what, out)
        print(f"varlen flash refused seq_lens {what}")
    a = FE._valid()
    OPS.flash_fwd(a["q"], a["k"], a["v"], a["o"], False, i32(64, 3))
    assert (a["o"] == 0).all()
    # keyword form; a [B, 1] shape with B elements is accepted
    OPS.flash_fwd(a["q"], a["k"], a["v"], a["o"], causal=True,
                  seq_lens=i32(1, 64).view(2, 1))


# ---- CPU: emulation of the length-aware kernels and single defects ---------------

def _rows(t, n, lim):
    """rows 0 .. n-1 of [1,h,S,dh] with rows >= lim zero (the guarded loads;
    n may pass S)"""
    out = t.new_zeros(t.shape[:2] + (n, t.shape[3]))
    m = min(lim, n, t.shape[2])
    out[:, :, :m] = t[:, :, :m]
    return out


def emulate(name, mutant=None):
    """The four length-aware kernels in fp32, one batch element at a time:
    L replaces S in the row guards, the key mask and the loop bounds; rows
    >= L are stored as zeros. Returns o, lse, dq, dk, dv as the ops do."""
    c = CASES[name]
    q, k, v, dout = inputs(name)
    B, S, h, dh = c["B"], c["S"], c["h"], c["dh"]
    sc = 1.0 / math.sqrt(dh)
    kvm = FE.kv_map(c)
    T = lambda t: t.transpose(-1, -2)
    o = torch.zeros(B, h, S, dh)
    lse = torch.zeros(B, h, S)
    dq, dk, dv = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(o)
    for b in range(B):
        L = c["lens"][(b + 1) % B if mutant == "next_batch_length" else b]
        if L == 0:
            continue
        Q, K, V, dO = (FE._f(t[b:b + 1]) for t in (q, k, v, dout))
        K, V = K[:, kvm], V[:, kvm]
        # ---- forward: rows < nq computed, keys < Lk visible
        nq = S if mutant == "dead_row_attends" else L
        Lk = min(S, L + 1) if mutant == "key_at_L_visible" else L
        nkv = Lk // 64 * 64 if mutant == "loop_bound_rounded_down" else Lk
        Qr = _rows(Q, nq, nq)
        qi = torch.arange(nq)[:, None]
        m = Qr.new_full(Qr.shape[:3], float("-inf"))
        l = Qr.new_zeros(Qr.shape[:3])
        acc = torch.zeros_like(Qr)
        for k0 in range(0, nkv, 64):
            kv = torch.arange(k0, k0 + 64)[None, :]
            valid = (kv < Lk).expand(nq, 64)
            if c["causal"]:
                valid = valid & (kv <= qi)
            Kt = _rows(K, k0 + 64, Lk)[:, :, k0:].contiguous()
            Vt = _rows(V, k0 + 64, Lk)[:, :, k0:].contiguous()
            s = (Qr @ T(Kt)) * sc
            s = torch.where(valid, s, torch.full_like(s, -1e30))
            mn = torch.maximum(m, s.amax(dim=-1))
            alpha = torch.exp(m - mn)
            m = mn
            p = torch.exp(s - mn[..., None])
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + FE.rbf(p) @ Vt
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        o[b, :, :nq] = FE.rbf(acc * inv[..., None])[0]
        lse[b, :, :nq] = (m + torch.log(l.clamp_min(1e-30)))[0]
        if mutant in FWD_ONLY:
            continue
        # ---- backward on the honest forward of this batch element; dk/dv
        # walk 32-row q tiles over rows < nq2 (padded rows carry the stored
        # o = 0 and lse = 0)
        nq2 = S if mutant == "dkv_takes_padded_q_rows" else L
        cut = lambda t, n: t[:, :, :n].contiguous()
        Qn, dOn = cut(Q, nq2), cut(dO, nq2)
        Ln = cut(lse[b:b + 1, :, :, None], nq2)
        dn = (dOn * cut(o[b:b + 1], nq2)).sum(-1)[..., None]
        KL, VL = cut(K, L), cut(V, L)
        keep = torch.ones(nq2, L, dtype=torch.bool)
        keep = keep.tril() if c["causal"] else keep

        def p_ds(Qr, dOr, Lr, dr, Kc, Vc, kp):
            p = torch.where(kp, torch.exp((Qr @ T(Kc)) * sc - Lr),
                            torch.zeros(()))
            return p, p * (dOr @ T(Vc) - dr) * sc

        acc = torch.zeros(1, h, L, dh)
        QL, dOL, LL, dL = cut(Qn, L), cut(dOn, L), cut(Ln, L), cut(dn, L)
        for k0 in range(0, L, 64):
            k1 = min(L, k0 + 64)
            _, ds = p_ds(QL, dOL, LL, dL, KL[:, :, k0:k1], VL[:, :, k0:k1],
                         keep[:L, k0:k1])
            acc = acc + FE.rbf(ds) @ KL[:, :, k0:k1]
        dq[b, :, :L] = FE.rbf(acc)[0]
        ak, av = torch.zeros(1, h, L, dh), torch.zeros(1, h, L, dh)
        for q0 in range(0, nq2, 32):
            r = slice(q0, min(nq2, q0 + 32))
            p, ds = p_ds(Qn[:, :, r], dOn[:, :, r], Ln[:, :, r], dn[:, :, r],
                         KL, VL, keep[r])
            av = av + T(FE.rbf(p)) @ dOn[:, :, r]
            ak = ak + T(FE.rbf(ds)) @ Qn[:, :, r]
        dk[b, :, :L], dv[b, :, :L] = FE.rbf(ak)[0], FE.rbf(av)[0]
    back = lambda t: t.permute(0, 2, 1, 3).to(BF16)
    return dict(o=back(o), lse=lse.reshape(B * h, S), dq=back(dq),
                dk=back(dk), dv=back(dv))


FWD_ONLY = ("key_at_L_visible", "dead_row_attends", "loop_bound_rounded_down")
# mutant -> (the cases that reach it, the outputs it is judged on)
MUTANTS = {
    # needs a length below S; lse is the sharp check for one extra key
    "key_at_L_visible": (
        [n for n in CASES if not CASES[n]["causal"]], ("lse",)),
    "next_batch_length": (list(CASES), ("o", "lse", "dq", "dk", "dv")),
    "dead_row_attends": (list(CASES), ("o", "lse")),
    # needs a length that is no multiple of 64
    "loop_bound_rounded_down": (list(CASES), ("o", "lse")),
    "dkv_takes_padded_q_rows": (
        [n for n in CASES if not CASES[n]["causal"]], ("dk", "dv")),
}


def test_bounds_admit_varlen_emulation():
    top = {}
    for name in CASES:
        c = CASES[name]
        got = emulate(name)
        r = ratios(name, got)
        print(f"varlen emulated {name}: "
              + ", ".join(f"{t} {x:.3f}" for t, x in r.items()))
        for t, x in r.items():
            assert x <= 1.0, f"{name}: honest fp32 {t} is {x:.3f} x the bound"
            top[t] = max(top.get(t, 0.0), x)
        # the same arithmetic as the dense emulation on the slices
        q, k, v, dout = inputs(name)
        lse = got["lse"].reshape(c["B"], c["h"], c["S"])
        for b, L in enumerate(c["lens"]):
            if L == 0:
                continue
            cb = slice_case(c, L)
            sl = lambda t: t[b:b + 1, :L]
            o_b, lse_b = FE.emulate_fwd(cb, sl(q), sl(k), sl(v))
            assert torch.equal(o_b, sl(got["o"])), (name, b)
            assert torch.equal(lse_b, lse[b, :, :L]), (name, b)
            grads = FE.emulate_bwd(cb, sl(q), sl(k), sl(v), sl(dout), o_b,
                                   lse_b)
            for tag, g in zip(("dq", "dk", "dv"), grads):
                assert torch.equal(g, sl(got[tag])), (name, b, tag)
    print(f"varlen emulated worst: {top}")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bounds_reject_varlen(mutant):
    names, outputs = MUTANTS[mutant]
    assert names
    best = 0.0
    for name in names:
        r = ratios(name, emulate(name, mutant))
        best = max(best, max(r[t] for t in outputs))
    print(f"varlen mutant {mutant}: {best:.1f} x the bound")
    assert best > 4.0, f"{mutant} reaches only {best:.2f} x the bound"
