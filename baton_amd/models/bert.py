"""BERT-base masked-LM on the HIP op layer (BASELINE.json config 3:
"BERT-base masked-LM fine-tune, 8 clients, FedAvg E=5").

Every hot op is a gfx950 kernel: QKV/projection/FFN Linears are MFMA GEMMs
(fused fp32-bias epilogue), attention is batched MFMA GEMMs around the
fused-scale softmax kernel (ops/functional.attention), LayerNorm and GELU
are the norm/elementwise kernels, the MLM loss is the fused log-softmax CE
over gathered masked positions, and the optimizer is the fused Adam.
Token/position embeddings are torch gathers (index ops, not in the
hand-written hot-op list).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from baton_amd.ops import functional as BF
from baton_amd.ops.modules import BatonGELU, BatonLayerNorm, BatonLinear
from baton_amd.runtime.local import LocalTrainer
from baton_amd.utils.config import TrainConfig


@dataclass
class BertConfig:
    # vocab padded to a multiple of 64 (true BERT vocab is 30522) so the
    # decoder GEMM rows stay 16-B aligned for glds staging — standard
    # tensor-core practice; labels never reference the 6 pad ids.
    vocab_size: int = 30528
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    max_positions: int = 512
    layer_norm_eps: float = 1e-12


class BertSelfAttention(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        self.qkv = BatonLinear(cfg.hidden, 3 * cfg.hidden)
        self.proj = BatonLinear(cfg.hidden, cfg.hidden)

    def forward(self, x, seq_lens=None):
        B, S, H = x.shape
        # packed QKV consumed as strided views — no permute copies on
        # either pass (AttnPackedFn writes dqkv slices in place)
        qkv = self.qkv(x).view(B, S, 3, self.heads, self.head_dim)
        o = BF.attention_qkv(qkv, causal=False,
                             seq_lens=seq_lens)              # [B, S, h, dh]
        return self.proj(o.reshape(B, S, H))


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.attn = BertSelfAttention(cfg)
        self.ln1 = BatonLayerNorm(cfg.hidden, eps=cfg.layer_norm_eps)
        self.fc1 = BatonLinear(cfg.hidden, cfg.ffn)
        self.act = BatonGELU()
        self.fc2 = BatonLinear(cfg.ffn, cfg.hidden)
        self.ln2 = BatonLayerNorm(cfg.hidden, eps=cfg.layer_norm_eps)

    def forward(self, x, seq_lens=None):
        # post-LN, BERT style; residual adds fused into the LN kernels
        # (layer_norm_add: one pass writes z = x + sub(x) and normalizes it)
        x = BF.layer_norm_add(self.attn(x, seq_lens), x, self.ln1.weight,
                              self.ln1.bias, self.ln1.eps)
        x = BF.layer_norm_add(self.fc2(self.act(self.fc1(x))), x,
                              self.ln2.weight, self.ln2.bias, self.ln2.eps)
        return x


class BertForMaskedLM(nn.Module):
    """Encoder + MLM head. ``forward(input_ids)`` returns hidden states;
    ``mlm_loss`` gathers the masked positions and applies the fused CE.

    Right-padded batches: ``forward(input_ids, seq_lens)`` with an int32 [B]
    tensor of live lengths on the ids' device (``lengths_from_mask`` builds
    and validates it from an attention mask). No live token then attends to
    a pad token, so the hidden states at live positions do not depend on
    what the padded positions hold; the hidden states at padded positions
    are not meaningful and their labels must be -100. ``train_round(ids,
    seq_lens, labels)`` trains on such data: LocalTrainer calls
    ``model(ids, seq_lens)``. That path runs eagerly, since the captured
    per-minibatch graph step takes a single input."""

    name = "bert-base-mlm"

    def __init__(self, cfg: Optional[BertConfig] = None,
                 train_config: Optional[TrainConfig] = None):
        super().__init__()
        self.cfg = cfg = cfg or BertConfig()
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos_emb = nn.Embedding(cfg.max_positions, cfg.hidden)
        self.emb_ln = BatonLayerNorm(cfg.hidden, eps=cfg.layer_norm_eps)
        self.encoder = nn.ModuleList(BertLayer(cfg) for _ in range(cfg.layers))
        self.head_fc = BatonLinear(cfg.hidden, cfg.hidden)
        self.head_act = BatonGELU()
        self.head_ln = BatonLayerNorm(cfg.hidden, eps=cfg.layer_norm_eps)
        self.decoder = BatonLinear(cfg.hidden, cfg.vocab_size)
        tc = train_config or TrainConfig(optimizer="adam", lr=5e-5)
        self._trainer = LocalTrainer(tc, loss_fn=self.mlm_loss)

    def forward(self, input_ids: torch.Tensor,
                seq_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, S = input_ids.shape
        pos = torch.arange(S, device=input_ids.device)
        x = self.tok_emb(input_ids) + self.pos_emb(pos)[None, :, :]
        x = self.emb_ln(x)
        if seq_lens is not None:
            seq_lens = seq_lens.to(torch.int32).contiguous()
        for layer in self.encoder:
            x = layer(x, seq_lens)
        return x

    def mlm_logits(self, hidden: torch.Tensor, mask_positions: torch.Tensor):
        """Gather masked positions ([Nmask] flat indices into [B*S]) and
        decode to vocab logits — only masked tokens pay the vocab GEMM."""
        H = hidden.shape[-1]
        flat = hidden.reshape(-1, H)
        sel = flat.index_select(0, mask_positions)
        sel = self.head_ln(self.head_act(self.head_fc(sel)))
        return self.decoder(sel)

    def mlm_loss(self, hidden: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """labels: [B, S] int64, -100 on unmasked positions (HF convention).
        Only the masked rows go through the vocab GEMM + CE."""
        flat = labels.reshape(-1)
        mask_positions = (flat != -100).nonzero(as_tuple=True)[0]
        logits = self.mlm_logits(hidden, mask_positions)
        return BF.cross_entropy(logits.contiguous(), flat[mask_positions])

    def train_round(self, *data, n_epoch: int = 1) -> List[float]:
        return self._trainer(self, data, n_epoch)


def bert_base(train_config: Optional[TrainConfig] = None) -> BertForMaskedLM:
    return BertForMaskedLM(BertConfig(), train_config)


def bert_tiny(train_config: Optional[TrainConfig] = None) -> BertForMaskedLM:
    """Small config for CPU tests / quick GPU checks."""
    cfg = BertConfig(vocab_size=512, hidden=64, layers=2, heads=4, ffn=128,
                     max_positions=64)
    m = BertForMaskedLM(cfg, train_config)
    m.name = "bert-tiny-mlm"
    return m


PAD_ID = 1   # pad token of make_synthetic_mlm(var_len=True); 0 is [MASK]


def lengths_from_mask(attention_mask: torch.Tensor) -> torch.Tensor:
    """Host-side, data-preparation time: an attention mask [B, S] of ones
    followed by zeros (right padding) -> int32 lengths [B] on the mask's
    device, the form ``seq_lens`` takes everywhere below. This is where range
    and right padding are validated (the kernels only clamp): raises
    ValueError on values other than 0 / 1, on left padding and on holes."""
    m = attention_mask
    if m.dim() != 2:
        raise ValueError(f"attention_mask must be [B, S], got {tuple(m.shape)}")
    if m.dtype.is_floating_point or m.dtype == torch.bool:
        vals = m.to(torch.float64)
    else:
        vals = m.to(torch.int64)
    if not bool(((vals == 0) | (vals == 1)).all()):
        raise ValueError("attention_mask may hold only 0 and 1")
    live = vals != 0
    lens = live.sum(dim=1)
    S = m.shape[1]
    expect = torch.arange(S, device=m.device)[None, :] < lens[:, None]
    if not bool((live == expect).all()):
        bad = (live != expect).any(dim=1).nonzero()[0].item()
        raise ValueError(
            f"attention_mask row {bad} is not ones followed by zeros: only "
            "right padding can be expressed as a length")
    return lens.to(torch.int32)


def make_synthetic_mlm(
    n_samples: int, seq_len: int, vocab_size: int = 30522,
    mask_frac: float = 0.15, seed: int = 0, var_len: bool = False,
):
    """Synthetic MLM data (no network for real corpora): random token ids;
    ~15% of positions masked (token replaced by id 0 = [MASK]); labels [n,S]
    hold the original token there and -100 elsewhere (HF convention).

    ``var_len=True`` returns ``(ids, seq_lens, labels)`` instead: lengths
    drawn uniformly in [1, seq_len] (int32 [n]), live tokens in
    [2, vocab_size), ``PAD_ID`` in the padded positions and -100 labels
    there, and at least one masked live position per sample."""
    g = torch.Generator().manual_seed(seed)
    if var_len:
        ids = torch.randint(2, vocab_size, (n_samples, seq_len), generator=g)
        lens = torch.randint(1, seq_len + 1, (n_samples,), generator=g)
        live = torch.arange(seq_len)[None, :] < lens[:, None]
        mask = (torch.rand(n_samples, seq_len, generator=g) < mask_frac) & live
        mask[:, 0] |= ~mask.any(dim=1)   # position 0 is live in every sample
        labels = torch.full_like(ids, -100)
        labels[mask] = ids[mask]
        masked_ids = ids.masked_fill(mask, 0).masked_fill(~live, PAD_ID)
        return masked_ids, lens.to(torch.int32), labels
    ids = torch.randint(1, vocab_size, (n_samples, seq_len), generator=g)
    mask = torch.rand(n_samples, seq_len, generator=g) < mask_frac
    mask[:, 0] |= ~mask.any(dim=1)   # every sample has >= 1 masked position
    labels = torch.full_like(ids, -100)
    labels[mask] = ids[mask]
    masked_ids = ids.masked_fill(mask, 0)
    return masked_ids, labels
