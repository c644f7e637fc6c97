"""Right-padded causal-LM batches: ``LlamaForCausalLM(ignore_index=-100)``,
``forward(input_ids, seq_lens)``, ``make_synthetic_clm(var_len=True)`` and
``validate_labels``.

Under a causal mask with right padding a live query never sees a padded key,
so hidden states and adapter gradients at live positions do not depend on what
the padded positions hold, with or without ``seq_lens``; what makes training
on such a batch correct is that the padded labels are ignored. The tests hold
the model to exactly that: bit-equal results under two paddings, a loss that
*does* move with the padding when nothing is ignored, and the padded-batch
loss against per-sequence runs of the trimmed sequences.

The LoRA B matrices start at zero, which makes every A gradient zero; the
tests give B small random values first so that all adapter gradients carry
signal.

Padded batch vs per-sequence runs (CPU, fp32): the tolerance is 4x the
discrepancy of the same identity for the unmodified dense model on a
full-length batch against its per-sample runs, which is measured in the test
(the noise floor of the reference: different GEMM shapes, different reduction
order). Measured: floor 4.77e-7, which is one fp32 ulp of the loss of about
6.2, so the tolerance is 1.91e-6; the padded batch against the trimmed runs
differs by 6.06e-7, the same with and without ``seq_lens``. Over eight other
seeds the floor was 1.2e-7 to 6.0e-7 and the padded discrepancy 9e-9 to
1.0e-6: both are rounding of an fp32 loss, not a property of the padding."""

import pytest
import torch

from baton_amd.models.llama import (
    LlamaForCausalLM, llama_tiny_config, make_synthetic_clm)
from baton_amd.ops import functional as BF

DEV = "cuda:0"


def tiny(seed, ignore_index=None):
    torch.manual_seed(seed)
    m = LlamaForCausalLM(llama_tiny_config(), ignore_index=ignore_index)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "lora_b" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return m


def repad(ids, lens, vocab, seed):
    """The same live tokens over random padding."""
    g = torch.Generator().manual_seed(seed)
    live = torch.arange(ids.shape[1])[None, :] < lens[:, None].long()
    noise = torch.randint(0, vocab, ids.shape, generator=g)
    return torch.where(live, ids, noise)


def loss_and_grads(m, ids, lens, labels):
    m.zero_grad(set_to_none=True)
    h = m(ids) if lens is None else m(ids, lens)
    loss = m.lm_loss(h, labels)
    loss.backward()
    return loss.detach(), [p.grad.detach().clone() for p in m.lora_parameters()]


# ---- CPU ---------------------------------------------------------------------

def test_validate_labels():
    C = 10
    good = torch.tensor([[0, 9, 3], [0, 0, 5]])
    assert BF.validate_labels(good, C, 0) is good
    assert BF.validate_labels(good, C, None) is good
    BF.validate_labels(torch.tensor([-100, 4, -100]), C, -100)
    for bad in (C, -1, -100):
        lab = good.clone()
        lab[0, 1] = bad
        with pytest.raises(ValueError, match=rf"label {bad} at index \(0, 1\)"):
            BF.validate_labels(lab, C, 0)
    # the first offender is the one named
    lab = torch.tensor([3, -100, 12, -1])
    with pytest.raises(ValueError, match=r"label 12 at index \(2,\)"):
        BF.validate_labels(lab, C, -100)
    with pytest.raises(ValueError, match=r"label -100 at index \(1,\)"):
        BF.validate_labels(lab, C, None)


def test_make_synthetic_clm_var_len():
    from baton_amd.models.llama import PAD_ID

    V, S, N = 512, 24, 64
    ids, lens, labels = make_synthetic_clm(N, S, V, seed=3, var_len=True)
    assert ids.shape == labels.shape == (N, S) and lens.shape == (N,)
    assert ids.dtype == labels.dtype == torch.int64
    assert lens.dtype == torch.int32
    assert int(lens.min()) >= 2 and int(lens.max()) <= S
    assert len(set(lens.tolist())) > 4, "lengths are meant to vary"
    live = torch.arange(S)[None, :] < lens[:, None].long()
    assert torch.equal(labels[live], ids[live])
    assert bool((labels[~live] == -100).all())
    assert bool((ids[~live] == PAD_ID).all())
    assert bool(((ids >= 0) & (ids < V)).all())
    BF.validate_labels(labels, V, -100)
    # the dense form is what it was
    a, b = make_synthetic_clm(N, S, V, seed=3)
    assert torch.equal(a, b) and a.shape == (N, S)
    assert torch.equal(a[live], ids[live])


def test_llama_tiny_trains_on_padded_batches():
    m = tiny(11, ignore_index=-100)
    cfg = m.cfg
    ids, lens, labels = make_synthetic_clm(6, 24, cfg.vocab_size, var_len=True)
    base = m.layers[0].attn.q_proj.weight.detach().clone()
    a_before = m.layers[0].attn.q_proj.lora_a.detach().clone()
    hist = m.train_round(ids, lens, labels, n_epoch=2)
    assert len(hist) == 2 and all(v == v and abs(v) < 1e4 for v in hist), hist
    assert torch.equal(base, m.layers[0].attn.q_proj.weight.detach())
    assert not torch.equal(a_before, m.layers[0].attn.q_proj.lora_a.detach())


def test_padding_independence():
    m = tiny(12, ignore_index=-100)
    V = m.cfg.vocab_size
    ids, lens, labels = make_synthetic_clm(4, 24, V, seed=5, var_len=True)
    assert int(lens.min()) < 24
    ids2 = repad(ids, lens, V, seed=6)
    assert not torch.equal(ids, ids2)
    for sl in (lens, None):
        l1, g1 = loss_and_grads(m, ids, sl, labels)
        l2, g2 = loss_and_grads(m, ids2, sl, labels)
        assert torch.isfinite(l1) and torch.equal(l1, l2), (sl is None, l1, l2)
        assert any(bool(g.abs().sum() > 0) for g in g1)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)
    # without ignored labels the pad tokens are trained on: the loss moves
    # with the padding (the dense loss needs class labels, so the ids)
    m.ignore_index = None
    d1, _ = loss_and_grads(m, ids, None, ids)
    d2, _ = loss_and_grads(m, ids2, None, ids2)
    assert not torch.equal(d1, d2)
    assert not torch.equal(d1, l1)


def _per_sequence(m, ids, lens):
    """sum_b n_b loss_b / sum_b n_b over dense B = 1 runs of ids[b, :L_b]."""
    num, den = 0.0, 0
    for b in range(ids.shape[0]):
        L = int(lens[b])
        seq = ids[b:b + 1, :L].contiguous()
        with torch.no_grad():
            lb = m.lm_loss(m(seq), seq)
        num += (L - 1) * lb.double().item()
        den += L - 1
    return num / den


def test_padded_batch_equals_per_sequence_runs():
    m = tiny(13)
    V, B, S = m.cfg.vocab_size, 4, 24
    # the reference's own noise floor: the dense model, a full-length batch
    full, _ = make_synthetic_clm(B, S, V, seed=8)
    with torch.no_grad():
        batch = m.lm_loss(m(full), full).double().item()
    floor = abs(batch - _per_sequence(m, full, torch.full((B,), S)))
    tol = 4 * floor

    ids, lens, labels = make_synthetic_clm(B, S, V, seed=9, var_len=True)
    want = _per_sequence(m, ids, lens)          # dense, trimmed
    m.ignore_index = -100
    for sl in (lens, None):
        with torch.no_grad():
            got = m.lm_loss(m(ids) if sl is None else m(ids, sl), labels)
        diff = abs(got.double().item() - want)
        print(f"llama_varlen padded vs per-sequence: floor {floor:.3e} "
              f"diff {diff:.3e} (seq_lens: {sl is not None})")
        assert diff <= tol, (diff, floor, tol)


# ---- GPU ---------------------------------------------------------------------

def tiny_gpu(seed, ignore_index=None):
    m = tiny(seed, ignore_index).to(DEV).to(torch.bfloat16)
    m.rope_cos = m.rope_cos.float()
    m.rope_sin = m.rope_sin.float()
    return m


def _gpu_batch(m):
    """S = 96 spans two 64-key flash tiles; lengths on both sides of the tile
    edge, one minimal."""
    V, S = m.cfg.vocab_size, 96
    lens = torch.tensor([96, 70, 33, 2], dtype=torch.int32)
    ids, _ = make_synthetic_clm(4, S, V, seed=21)
    live = torch.arange(S)[None, :] < lens[:, None].long()
    labels = ids.masked_fill(~live, -100)
    ids1 = ids.masked_fill(~live, 0)
    ids2 = repad(ids, lens, V, seed=22)
    return ids1.to(DEV), ids2.to(DEV), lens.to(DEV), labels.to(DEV), live


@pytest.mark.gpu
def test_gpu_hidden_states_at_live_positions():
    """dh = 32, GQA 2, causal: the length-aware flash path. Masked keys
    contribute exactly 0 to the online softmax, so the live rows are the
    dense ones bit for bit, and they do not see the padding."""
    m = tiny_gpu(14)
    ids1, ids2, lens, _, live = _gpu_batch(m)
    with torch.no_grad():
        h_len = m(ids1, lens).cpu()
        h_dense = m(ids1).cpu()
        h_len2 = m(ids2, lens).cpu()
        h_dense2 = m(ids2).cpu()
    assert torch.isfinite(h_len[live]).all()
    assert torch.equal(h_len[live], h_dense[live])
    assert torch.equal(h_len[live], h_len2[live])
    assert torch.equal(h_dense[live], h_dense2[live])
    assert not torch.equal(h_dense[~live], h_dense2[~live])


@pytest.mark.gpu
def test_gpu_training_step_and_padding():
    """One step with ignore_index = -100: finite loss and adapter gradients.
    Two paddings give bit-equal live logits, hence equal row losses; the loss
    sums them with unordered atomics, so each is within (n + 2) 2^-24 mean|r|
    of the exact mean (tests/test_ce_exact.py; r >= 0, so mean|r| is the loss)
    and the two agree within twice that."""
    m = tiny_gpu(15, ignore_index=-100)
    ids1, ids2, lens, labels, live = _gpu_batch(m)
    l1, g1 = loss_and_grads(m, ids1, lens, labels)
    l2, g2 = loss_and_grads(m, ids2, lens, labels)
    l3, _ = loss_and_grads(m, ids2, None, labels)
    assert all(torch.isfinite(v) for v in (l1, l2, l3)), (l1, l2, l3)
    assert all(bool(torch.isfinite(g).all()) for g in g1 + g2)
    assert any(bool(g.float().abs().sum() > 0) for g in g1)
    n = int(live[:, 1:].sum())
    top = max(l1.item(), l2.item(), l3.item())
    lim = 2 * (n + 2) * 2.0 ** -24 * top
    print(f"llama_varlen gpu losses {l1.item():.7f} {l2.item():.7f} "
          f"{l3.item():.7f}, bound {lim:.3e}")
    assert abs(l1.item() - l2.item()) <= lim
    assert abs(l1.item() - l3.item()) <= lim
    hist = m.train_round(ids1, lens, labels, n_epoch=1)
    assert hist[0] == hist[0] and abs(hist[0]) < 1e4, hist
