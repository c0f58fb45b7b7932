"""Restatement of DESIGN.md section 4d (adaptive top-k KV selection in the geo decoder) for the tests: the cut of a pass into
groups, the sampled rows, the scores in float64 from the given bf16 values, the selection with its tie rule, the validity check of a
selection somebody else made, and the geo decoder of the oracle with its cross-attention restricted to a GIVEN index table.
Written from the text of section 4d, not from csrc/kvsel_kernels.hip."""
import copy

import numpy as np
import torch

DEFAULT_GROUP, DEFAULT_STRIDE = 8192, 64


def upstream_topk(num_latents):
    """the -1 rule [UPSTREAM-RECALLED]"""
    return 1024 if num_latents == 3072 else 256 if num_latents == 512 else num_latents // 3


def groups(n, group):
    """(first row, rows) of the groups of n consecutive rows; the last one may be shorter"""
    return [(g0, min(group, n - g0)) for g0 in range(0, n, group)]


def sample_rows(rows, stride):
    """offsets r inside a group with r % stride == 0 (a tail shorter than the stride: row 0 alone)"""
    return list(range(0, rows, stride))


def scores(q, k, group, stride):
    """q [H, n, 64], k [H, N, 64] (any float dtype; taken as they are) -> float64 (s [groups, H, N], a [groups, H, N], S [groups]):
    s = q-bar . k with q-bar the mean of the group's sampled rows; a = sum_d mean_s |q_sd| |k_d|, the magnitude the fp32
    accumulation error of an implementation scales with; S = samples per group"""
    q, k = q.detach().cpu().double(), k.detach().cpu().double()
    s_out, a_out, S_out = [], [], []
    for g0, rows in groups(q.shape[1], group):
        rr = torch.tensor([g0 + r for r in sample_rows(rows, stride)])
        qs = q[:, rr]                                            # [H, S, 64]
        s_out.append(torch.einsum("hd,hnd->hn", qs.mean(1), k))
        a_out.append(torch.einsum("hd,hnd->hn", qs.abs().mean(1), k.abs()))
        S_out.append(len(rr))
    return torch.stack(s_out).numpy(), torch.stack(a_out).numpy(), np.array(S_out)


def accumulation_eps(a, S):
    """per key: (S + 66) 2^-24 sum_d mean_s |q_sd| |k_d| -- S additions and a division for the mean, 64 multiply-adds for the dot,
    each with a relative rounding error of 2^-24, on terms whose magnitudes sum to `a`"""
    return (S[:, None, None] + 66.0) * 2.0 ** -24 * a


def select(s, k):
    """s [..., N] (float32 or float64) -> int64 [..., k]: the k keys of largest score in ascending key index.  Equal scores go to
    the lower index; a NaN ranks below every number, NaNs among themselves by index."""
    s = np.asarray(s)
    flat = s.reshape(-1, s.shape[-1])
    out = np.empty((flat.shape[0], k), np.int64)
    ar = np.arange(s.shape[-1])
    for i, row in enumerate(flat):
        nan = np.isnan(row)
        order = np.lexsort((ar, np.where(nan, 0.0, -row), nan))      # not-NaN first, then descending score, then ascending index
        out[i] = np.sort(order[:k])
    return out.reshape(s.shape[:-1] + (k,))


def check_selection(idx, s, eps, k, cap=0.01):
    """idx int [groups, H, k] against float64 scores s and per-key eps [groups, H, N]: ascending and distinct indices inside the key
    range; with t the k-th largest score, every selected key has s >= t - 2 eps and every other key s <= t + 2 eps; keys with
    |s - t| <= 2 eps are unconstrained and must not exceed `cap` of N in any (group, head) (cap None: not checked).  Returns the
    largest unconstrained share."""
    idx = np.asarray(idx).astype(np.int64)
    G, H, N = s.shape
    assert idx.shape == (G, H, k), (idx.shape, (G, H, k))
    assert idx.min() >= 0 and idx.max() < N
    assert (np.diff(idx, axis=-1) > 0).all(), "indices are not ascending and distinct"
    assert not np.isnan(s).any()
    t = np.sort(s, axis=-1)[..., N - k][..., None]
    chosen = np.zeros(s.shape, bool)
    np.put_along_axis(chosen, idx, True, axis=-1)
    bad_in = chosen & (s < t - 2 * eps)
    bad_out = ~chosen & (s > t + 2 * eps)
    assert not bad_in.any(), "%d selected keys lie below the k-th largest score by more than 2 eps" % bad_in.sum()
    assert not bad_out.any(), "%d keys above the k-th largest score by more than 2 eps were not selected" % bad_out.sum()
    free = (np.abs(s - t) <= 2 * eps).sum(-1) / N
    if cap is not None:
        assert free.max() <= cap, "%.4f of the keys of one (group, head) are within 2 eps of the threshold" % free.max()
    return float(free.max())


def topk_geo_decoder(geo_decoder, idx, group):
    """a copy of the oracle's CrossAttentionDecoder whose cross-attention runs, per group of `group` consecutive queries and per
    head, over the keys idx[group, head] only (idx: int [groups, H, k])"""
    from oracle import hy3d_torch as H
    import torch.nn.functional as F

    class TopKCrossAttention(H.QKVMultiheadCrossAttention):
        def forward(self, q, kv):
            _, n_ctx, _ = q.shape
            bs, n_data, width = kv.shape
            attn_ch = width // self.heads // 2
            q = q.view(bs, n_ctx, self.heads, -1)
            kv = kv.view(bs, n_data, self.heads, -1)
            k, v = torch.split(kv, attn_ch, dim=-1)
            q, k = self.q_norm(q), self.k_norm(k)
            q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
            table = torch.as_tensor(np.array(self.kv_idx), dtype=torch.long)
            cut = groups(n_ctx, self.kv_group)
            assert table.shape[0] == len(cut) and table.shape[1] == self.heads
            out = []
            for g, (g0, rows) in enumerate(cut):
                sel = table[g][None, :, :, None].expand(bs, -1, -1, k.shape[-1])
                out.append(F.scaled_dot_product_attention(q[:, :, g0:g0 + rows], k.gather(2, sel), v.gather(2, sel)))
            return torch.cat(out, dim=2).transpose(1, 2).reshape(bs, n_ctx, -1)

    dec = copy.deepcopy(geo_decoder)
    old = dec.cross_attn_decoder.attn.attention
    new = TopKCrossAttention.__new__(TopKCrossAttention)
    torch.nn.Module.__init__(new)
    new.heads, new.q_norm, new.k_norm = old.heads, old.q_norm, old.k_norm
    new.kv_idx, new.kv_group = idx, int(group)
    dec.cross_attn_decoder.attn.attention = new
    return dec.eval()


def oracle_qk(geo_decoder, queries, latents):
    """the fp32 q [H, n, 64] (after q_norm) and k [H, N, 64] (after k_norm) the oracle's cross-attention forms for `queries`
    [n, 3] and the decoded latents [1, N, W]"""
    blk = geo_decoder.cross_attn_decoder
    att = blk.attn.attention
    with torch.no_grad():
        x = geo_decoder.query_proj(geo_decoder.fourier_embedder(queries[None]).to(latents.dtype))
        q = blk.attn.c_q(blk.ln_1(x))
        kv = blk.attn.c_kv(blk.ln_2(latents))
        q = att.q_norm(q.view(1, q.shape[1], att.heads, -1))[0].permute(1, 0, 2)
        kv = kv.view(1, kv.shape[1], att.heads, -1)
        k = att.k_norm(kv[..., :kv.shape[-1] // 2])[0].permute(1, 0, 2)
    return q.contiguous(), k.contiguous()
