"""Per-sequence lengths outside the flash kernels: ``softmax_fwd`` with
``kv_len`` on every route, the materialized-scores path of ``attention_qkv``,
the CPU form of the wrappers, the BERT model and the data helpers. The flash
kernels themselves are in tests/test_attention_varlen.py; cases and inputs
are shared with it.

softmax_fwd(x, scale, causal_seq, kv_len, rows_per_len, q_period): row r has
entry e = r // rows_per_len and query position r % q_period; with
L = kv_len[e] its visible columns are c < L (and c <= r % causal_seq), and a
row whose query position is >= L is all zeros. Live rows are held to the
bound of tests/test_softmax_exact.py with the row's number of visible columns
n in place of C (the sum has n terms) and A over the visible columns:

    |y - ref| <= (store + (n + 8 + 6 A) 2^-23) ref     masked, dead: exactly 0

The cases are C = S, h = 1, one per route. bf16 C = 1032 is a multiple of 8
and so takes the vector path of the row-per-block kernel (as in
test_softmax_exact.py); C = 1027 covers its scalar path. Worst observed
error / bound on an MI355X: 0.992 bf16 (the store term), 0.068 fp32. Masked
columns of x hold NaN on the vector routes (whole vectors are loaded and
masked per element) and 1e4 on the scalar ones (which may not read them).
``softmax_bwd`` takes no lengths: y == 0 gives dx == 0, checked here.

Materialized-scores attention (fp32 inputs, or dh = 16) stores the scores,
the probabilities, dP and dS in the input dtype, so the flash bounds do not
apply. With u one rounding of that dtype (2^-8 bf16, 0 for fp32: an fp32
store is covered by the 2^-23 terms), A_q, eps_q, c as in test_flash_exact.py
and every product of error factors kept:

    d_q   = u A_q + eps_q                 one scaled score
    r_q   = (1 + u) e^(2 d_q) (1 + (S + 8 + 6 A_q) 2^-23) - 1   one stored p
    |o - ref|  <= u |ref| + (1 + u) ((1 + r_q)(1 + c) - 1) (P |V|)
    E_dP  = u |dP| + (dh + 2) 2^-23 |dO| |V|^T
    E_dot = sum_j (r_q P |dP| + (1 + r_q) P E_dP)
            + c sum_j (1 + r_q) P (|dP| + E_dP)
    pre   = sc (r_q P (|dP| + |delta|) + (1 + r_q) P (E_dP + E_dot))
            + 4 2^-23 sc (1 + r_q) P (|dP| + E_dP + |delta| + E_dot)
    E_dS  = pre + u (|dS| + pre)
    |dq - ref| <= u |ref| + (1 + u) (E_dS |K| + c (|dS| + E_dS) |K|)
    |dk - ref| <= u |ref| + (1 + u) (E_dS^T |Q| + c (|dS| + E_dS)^T |Q|)
    |dv - ref| <= u |ref| + (1 + u) (r_q P + c (1 + r_q) P)^T |dO|

The GEMMs multiply the padded rows of k, v and dout by exact zeros, so this
path needs them finite (the flash path never reads them); the padded rows of
o, dq, dk, dv must then be exactly 0. The CPU form of the wrappers rounds at
the same points, so the same bounds are checked without a GPU on bf16 inputs,
and the u = 0 form of the flash bounds on fp32 inputs."""

import contextlib
import functools
import math

import pytest
import torch

import test_attention_varlen as TV
import test_flash_exact as FE
import test_softmax_exact as SE
from baton_amd.ops import functional as BF

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = FE.DEV
BF16, FP32 = FE.BF16, FE.FP32
U, E23 = FE.U, FE.E23
SCALE = SE.SCALE

# ---- softmax_fwd with lengths ------------------------------------------------

# name -> (dtype, C = S, lens, kernel, vector path)
SM_CASES = {
    "bf16_96_scalar_wave": (BF16, 96, (96, 65, 31), "wave", False),
    "bf16_512_vector_wave": (BF16, 512, (512, 130), "wave", True),
    "fp32_256_vector_wave": (FP32, 256, (256, 129, 1), "wave", True),
    "bf16_1032_vector_block": (BF16, 1032, (1032, 517), "block", True),
    "bf16_1027_scalar_block": (BF16, 1027, (1027, 0, 514), "block", False),
    "bf16_1536_vector_block": (BF16, 1536, (1536, 1025, 7), "block", True),
}
SM_PARAMS = [(n, causal) for n in SM_CASES for causal in (False, True)]


@functools.lru_cache(maxsize=2)
def sm_inputs(name, causal):
    """x [B*S, S] with the masked columns poisoned, dy, the visible mask, the
    float64 reference and its bound. Never modified."""
    dtype, S, lens, kernel, vec = SM_CASES[name]
    assert SE.route(len(lens) * S, S, dtype)[:2] == (kernel, vec)
    B = len(lens)
    g = torch.Generator().manual_seed(31 * S + B)
    x = torch.randn(B * S, S, generator=g).mul(3.0)
    dy = torch.randn(B * S, S, generator=g).to(dtype)
    L = torch.tensor(lens).repeat_interleave(S)[:, None]
    qpos = (torch.arange(B * S) % S)[:, None]
    cols = torch.arange(S)[None, :]
    keep = (cols < L) & (qpos < L)
    if causal:
        keep = keep & (cols <= qpos)
    poison = float("nan") if vec else 1e4
    x = torch.where(keep, x, torch.full_like(x, poison)).to(dtype)
    live = keep.any(dim=1, keepdim=True)
    z = (SCALE * x.double()).masked_fill(~keep, float("-inf"))
    z = torch.where(live, z, torch.zeros_like(z))       # dead rows: ref 0
    ref = torch.softmax(z, dim=-1) * keep
    A = torch.where(keep, z, torch.zeros_like(z)).abs().amax(dim=-1,
                                                             keepdim=True)
    n = keep.sum(dim=1, keepdim=True)
    store = U if dtype == BF16 else 0.0
    lim = (store + (n + 8 + 6 * A) * E23) * ref
    return x, dy, keep, ref, lim


@pytest.mark.gpu
@pytest.mark.parametrize("name,causal", SM_PARAMS)
def test_softmax_kv_len(name, causal):
    dtype, S, lens, _, _ = SM_CASES[name]
    x, dy, keep, ref, lim = sm_inputs(name, causal)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    y = OPS.softmax_fwd(x.to(DEV), SCALE, S if causal else 0, kv_len, S, S)
    assert y.dtype == dtype and tuple(y.shape) == tuple(x.shape)
    yc = y.cpu()
    assert torch.isfinite(yc).all()
    assert (yc[~keep] == 0).all(), "masked columns and dead rows must be 0"
    r = SE.worst(yc, ref, lim)
    print(f"varlen softmax {name}{'_causal' if causal else ''}: "
          f"worst error / bound = {r:.4f}")
    assert r <= 1.0, f"forward error is {r:.3f} x the bound"
    # the backward needs no lengths: y == 0 gives dx == 0
    dx = OPS.softmax_bwd(y, dy.to(DEV), SCALE).cpu()
    assert (dx[~keep] == 0).all()
    rb = SE.worst(dx, *SE.bwd_reference(yc, dy, dtype))
    assert rb <= 1.0, f"backward error is {rb:.3f} x the bound"


@pytest.mark.gpu
def test_softmax_kv_len_none_is_the_plain_call():
    x = torch.randn(3 * 96, 96, device=DEV).to(BF16)
    for cs in (0, 96):
        assert torch.equal(OPS.softmax_fwd(x, SCALE, cs),
                           OPS.softmax_fwd(x, SCALE, cs, None, 0, 0))
        assert torch.equal(OPS.softmax_fwd(x, SCALE, cs),
                           OPS.softmax_fwd(x, scale=SCALE, causal_seq=cs))


@pytest.mark.gpu
def test_softmax_refuses_bad_kv_len():
    x = torch.zeros(2 * 64, 64, dtype=BF16, device=DEV)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=DEV)
    bad = {
        "int64": ((torch.tensor([64, 64], device=DEV), 64, 64),
                  "kv_len must be int32"),
        "strided": ((i32(64, 0, 64, 0)[::2], 64, 64),
                    "kv_len must be contiguous"),
        "cpu": ((torch.tensor([64, 64], dtype=torch.int32), 64, 64),
                "kv_len must be on"),
        "count": ((i32(64, 64, 64), 64, 64), "kv_len must have exactly"),
        "rows_not_a_multiple": ((i32(64, 64), 48, 64), "not a multiple"),
        "rows_per_len_0": ((i32(64, 64), 0, 64), "rows_per_len > 0"),
        "q_period_0": ((i32(64, 64), 64, 0), "q_period > 0"),
    }
    for what, (args, msg) in bad.items():
        with pytest.raises(RuntimeError, match=msg):
            OPS.softmax_fwd(x, SCALE, 0, *args)
        print(f"varlen softmax refused {what}")
    y = OPS.softmax_fwd(x, SCALE, 0, i32(64, 2), 64, 64)
    assert torch.equal(y[64, :3].float().cpu(), torch.tensor([0.5, 0.5, 0.0]))
    assert (y[64 + 2:] == 0).all()


# ---- materialized-scores attention ----------------------------------------------

def mat_reference(cb, q, k, v, dout, u):
    """float64 o, dq, dk, dv (dk, dv per q head) of one dense case and the
    bounds of the module docstring; everything [B,S,h,dh]."""
    S, dh = cb["S"], cb["dh"]
    sc = 1.0 / math.sqrt(dh)
    kvm = FE.kv_map(cb)
    Q, K, V, dO = FE.hf(q), FE.hf(k)[:, kvm], FE.hf(v)[:, kvm], FE.hf(dout)
    keep = FE.keep_mask(cb)
    T = lambda t: t.transpose(-1, -2)
    Sx = (sc * Q @ T(K)).masked_fill(~keep, float("-inf"))
    P = torch.softmax(Sx, dim=-1)
    Aq = (sc * Q.abs() @ T(K.abs())).masked_fill(~keep, 0.0).amax(
        dim=-1, keepdim=True)
    eps = (dh + 2) * E23 * Aq
    cc = (S + 4) * E23
    d = u * Aq + eps
    r = (1 + u) * torch.exp(2 * d) * (1 + (S + 8 + 6 * Aq) * E23) - 1
    o = P @ V
    lim_o = u * o.abs() + (1 + u) * ((1 + r) * (1 + cc) - 1) * (P @ V.abs())
    dP = dO @ T(V)
    E_dP = u * dP.abs() + (dh + 2) * E23 * (dO.abs() @ T(V.abs()))
    delta = (P * dP).sum(-1, keepdim=True)
    E_dot = (r * P * dP.abs() + (1 + r) * P * E_dP).sum(-1, keepdim=True) \
        + cc * ((1 + r) * P * (dP.abs() + E_dP)).sum(-1, keepdim=True)
    dS = sc * P * (dP - delta)
    pre = sc * (r * P * (dP.abs() + delta.abs())
                + (1 + r) * P * (E_dP + E_dot)) \
        + 4 * E23 * sc * (1 + r) * P * (dP.abs() + E_dP + delta.abs() + E_dot)
    E_dS = pre + u * (dS.abs() + pre)
    mag = dS.abs() + E_dS
    dq, dk, dv = dS @ K, T(dS) @ Q, T(P) @ dO
    lim_dq = u * dq.abs() + (1 + u) * (E_dS @ K.abs() + cc * mag @ K.abs())
    lim_dk = u * dk.abs() + (1 + u) * (T(E_dS) @ Q.abs()
                                       + cc * T(mag) @ Q.abs())
    lim_dv = u * dv.abs() + (1 + u) * (T(r * P + cc * (1 + r) * P)
                                       @ dO.abs())
    back = lambda t: t.permute(0, 2, 1, 3)
    return dict(o=back(o), lim_o=back(lim_o), dq=back(dq), lim_dq=back(lim_dq),
                dk=back(dk), lim_dk=back(lim_dk), dv=back(dv),
                lim_dv=back(lim_dv))


MAT_LENS = TV.CASES["s96_packed_qkv"]["lens"]


@functools.lru_cache(maxsize=None)
def mat_inputs(dtype, dh):
    """q, k, v, dout [3,96,2,dh] in ``dtype``, finite in every row."""
    g = torch.Generator().manual_seed(77 + dh)
    return tuple(torch.randn(3, 96, 2, dh, generator=g).add(s).to(dtype)
                 for s in (0.0, 0.0, 0.25, -0.25))


def run_qkv(q, k, v, dout, causal, lens, dev):
    qkv = torch.stack((q, k, v), dim=2).to(dev).requires_grad_(True)
    o = BF.attention_qkv(qkv, causal, seq_lens=lens)
    o.backward(dout.to(dev))
    g = qkv.grad.cpu()
    return dict(o=o.detach().cpu(), dq=g[:, :, 0], dk=g[:, :, 1], dv=g[:, :, 2])


def check_materialized(tag, got, q, k, v, dout, causal, lens, u):
    c = FE.case(96, 2, 2, q.shape[-1], causal, B=3)
    for b, L in enumerate(lens):
        for t in ("o", "dq", "dk", "dv"):
            assert (got[t][b, L:] == 0).all(), (tag, t, b)
        sl = lambda t: t[b:b + 1, :L]
        ref = mat_reference(dict(c, S=L, B=1), sl(q), sl(k), sl(v), sl(dout),
                            u)
        for t in ("o", "dq", "dk", "dv"):
            r = FE.worst(sl(got[t]), ref[t], ref["lim_" + t])
            print(f"varlen materialized {tag} b={b} {t}: {r:.4f}")
            assert r <= 1.0, f"{tag} b={b}: {t} error is {r:.3f} x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,dh", [(FP32, 32), (BF16, 16)])
def test_attention_qkv_materialized_varlen(dtype, dh, causal):
    q, k, v, dout = mat_inputs(dtype, dh)
    assert not BF._flash_eligible(q.to(DEV), k.to(DEV), v.to(DEV))
    lens = torch.tensor(MAT_LENS, dtype=torch.int32, device=DEV)
    got = run_qkv(q, k, v, dout, causal, lens, DEV)
    check_materialized(f"gpu {dtype} dh={dh}", got, q, k, v, dout, causal,
                       MAT_LENS, U if dtype == BF16 else 0.0)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,dh", [(FP32, 32), (BF16, 16)])
def test_attention_qkv_cpu_rounds_like_the_materialized_path(dtype, dh, causal):
    q, k, v, dout = mat_inputs(dtype, dh)
    lens = torch.tensor(MAT_LENS, dtype=torch.int32)
    got = run_qkv(q, k, v, dout, causal, lens, "cpu")
    check_materialized(f"cpu {dtype} dh={dh}", got, q, k, v, dout, causal,
                       MAT_LENS, U if dtype == BF16 else 0.0)


# ---- the wrappers on the CPU: fp32, the u = 0 form of the flash bounds ----------

@contextlib.contextmanager
def flash_bounds_without_bf16():
    """test_flash_exact's references with u = 0: fp32 data, no bf16 pack or
    store anywhere."""
    old = FE.U
    FE.U = 0.0
    try:
        yield
    finally:
        FE.U = old


def other_padding(c, *tensors):
    """The same live rows, other finite values in the padded ones."""
    g = torch.Generator().manual_seed(5)
    out = []
    for t in tensors:
        t = t.clone()
        for b, L in enumerate(c["lens"]):
            t[b, L:] = torch.randn(t[b, L:].shape, generator=g).mul(4.0)
        out.append(t)
    return out


@pytest.mark.parametrize("name", ["s200", "s200_causal"])
def test_wrappers_on_cpu(name):
    c = TV.CASES[name]
    B, S, h, kvh, dh = c["B"], c["S"], c["h"], c["kvh"], c["dh"]
    g = h // kvh
    base = tuple(t.float() for t in TV.inputs(name))
    lens = torch.tensor(c["lens"], dtype=torch.int32)

    def bshd(q, k, v, dout):
        q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = BF.attention_bshd(q, k, v, c["causal"], seq_lens=lens)
        o.backward(dout)
        return dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)

    def packed(q, k, v, dout):
        # k, v replicated per q head: the packed layout has no GQA, and the
        # gradients come out per q head like the reference
        kx = k.repeat_interleave(g, dim=2)
        vx = v.repeat_interleave(g, dim=2)
        return run_qkv(q, kx, vx, dout, c["causal"], lens, "cpu")

    for fn in (bshd, packed):
        got = fn(*base)
        again = fn(*other_padding(c, *base))
        top = {}
        for b, L in enumerate(c["lens"]):
            for t in ("o", "dq", "dk", "dv"):
                assert (got[t][b, L:] == 0).all(), (fn.__name__, t, b)
                # nothing in the padding reaches a live row
                assert torch.equal(got[t][b, :L], again[t][b, :L]), \
                    (fn.__name__, t, b)
            if L == 0:
                continue
            cb = TV.slice_case(c, L)
            sl = lambda t: t[b:b + 1, :L]
            with flash_bounds_without_bf16():
                f = FE.fwd_reference(cb, *(sl(t) for t in base[:3]))
                bw = FE.bwd_reference(cb, *(sl(t) for t in base),
                                      sl(got["o"]), f["lse"])
            ref = dict(o=(f["o"], f["lim_o"]), dq=(bw["dq"], bw["lim_dq"]))
            for t in ("dk", "dv"):
                r_, l_ = bw[t], bw["lim_" + t]
                if fn is bshd and g > 1:
                    # one fp32 sum of the g per-head terms
                    terms = r_.reshape(1, L, kvh, g, dh)
                    l_ = l_.reshape(1, L, kvh, g, dh).sum(3) \
                        + g * E23 * terms.abs().sum(3)
                    r_ = terms.sum(3)
                ref[t] = (r_, l_)
            for t, (r_, l_) in ref.items():
                top[t] = max(top.get(t, 0.0), FE.worst(sl(got[t]), r_, l_))
        print(f"varlen cpu {fn.__name__} {name}: "
              + ", ".join(f"{t} {x:.3f}" for t, x in top.items()))
        for t, x in top.items():
            assert x <= 1.0, f"{fn.__name__} {name}: {t} is {x:.3f} x the bound"


def test_seq_lens_none_is_unchanged_on_cpu():
    q, k, v, _ = (t.float() for t in TV.inputs("s96_packed_qkv"))
    qkv = torch.stack((q, k, v), dim=2)
    assert torch.equal(BF.attention_qkv(qkv, True),
                       BF.attention_qkv(qkv, True, seq_lens=None))
    full = torch.full((3,), 96, dtype=torch.int32)
    assert torch.equal(BF.attention_qkv(qkv, True),
                       BF.attention_qkv(qkv, True, seq_lens=full))


# ---- model and data helpers ----------------------------------------------------

def test_lengths_from_mask():
    from baton_amd.models.bert import lengths_from_mask

    m = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]])
    for mask in (m, m.bool(), m.float(), m.to(torch.int32)):
        lens = lengths_from_mask(mask)
        assert lens.dtype == torch.int32 and lens.tolist() == [4, 2, 1, 0]
    bad = {
        "left_padding": [[0, 0, 1, 1]],
        "hole": [[1, 0, 1, 0]],
        "trailing_one": [[1, 1, 0, 1]],
        "two": [[1, 2, 0, 0]],
        "negative": [[1, -1, 0, 0]],
        "fraction": [[1.0, 0.5, 0.0, 0.0]],
    }
    for what, rows in bad.items():
        with pytest.raises(ValueError):
            lengths_from_mask(torch.tensor([[1, 1, 1, 0]] + rows))
    with pytest.raises(ValueError):
        lengths_from_mask(torch.ones(4))


def test_make_synthetic_mlm_var_len():
    from baton_amd.models.bert import PAD_ID, make_synthetic_mlm

    ids0, labels0 = make_synthetic_mlm(16, 24, vocab_size=512, seed=3)
    g = torch.Generator().manual_seed(3)     # the default return is unchanged
    want = torch.randint(1, 512, (16, 24), generator=g)
    assert torch.equal(labels0[labels0 != -100], want[labels0 != -100])
    ids, lens, labels = make_synthetic_mlm(64, 24, vocab_size=512, seed=3,
                                           var_len=True)
    assert tuple(ids.shape) == (64, 24) == tuple(labels.shape)
    assert lens.dtype == torch.int32 and tuple(lens.shape) == (64,)
    assert lens.min() >= 1 and lens.max() <= 24
    assert len(set(lens.tolist())) > 4
    live = torch.arange(24)[None, :] < lens[:, None]
    assert (ids[~live] == PAD_ID).all() and (ids[live] != PAD_ID).all()
    assert (labels[~live] == -100).all()
    masked = labels != -100
    assert masked.any(dim=1).all(), "a sample without a masked live position"
    assert (ids[masked] == 0).all() and (labels[masked] >= 2).all()
    assert (ids[live & ~masked] >= 2).all()


def test_bert_tiny_cpu_step_with_seq_lens():
    from baton_amd.models.bert import bert_tiny, make_synthetic_mlm

    torch.manual_seed(8)
    m = bert_tiny()
    ids, lens, labels = make_synthetic_mlm(8, 32, vocab_size=512,
                                           var_len=True)
    hist = m.train_round(ids, lens, labels, n_epoch=1)
    assert len(hist) == 1 and math.isfinite(hist[0])
    # padding content cannot reach a live position
    m.eval()
    live = torch.arange(32)[None, :] < lens[:, None]
    other = torch.where(live, ids, torch.randint(2, 512, ids.shape))
    with torch.no_grad():
        a, b = m(ids, lens), m(other, lens)
        assert torch.equal(a[live], b[live])
        assert not torch.equal(m(ids)[live], m(other)[live])


@pytest.mark.gpu
def test_bert_hidden_states_ignore_padding():
    from baton_amd.models.bert import BertConfig, BertForMaskedLM

    torch.manual_seed(9)
    cfg = BertConfig(vocab_size=512, hidden=64, layers=2, heads=2, ffn=128,
                     max_positions=64)       # dh = 32: the flash path
    m = BertForMaskedLM(cfg).to(DEV).to(BF16).eval()
    B, S, lens = 3, 48, (48, 17, 1)
    g = torch.Generator().manual_seed(10)
    ids = torch.randint(2, 512, (B, S), generator=g)
    live = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    other = torch.where(live, ids, torch.randint(2, 512, (B, S), generator=g))
    assert (other != ids)[~live].any()
    ids, other, live = ids.to(DEV), other.to(DEV), live.to(DEV)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        a, b = m(ids, sl), m(other, sl)
        assert torch.isfinite(a[live]).all()
        assert torch.equal(a[live], b[live]), \
            "padding reached a live position despite seq_lens"
        # without lengths every token attends to the pad tokens
        assert not torch.equal(m(ids)[live], m(other)[live])
    # and a training step through the model runs
    m.train()
    labels = torch.full((B, S), -100, device=DEV)
    labels[:, 0] = ids[:, 0]
    loss = m.mlm_loss(m(ids, sl), labels)
    loss.backward()
    assert torch.isfinite(loss).item()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters()
               if p.grad is not None)
