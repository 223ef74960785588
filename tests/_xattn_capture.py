"""Shared by tests/golden/make_g18_alignment.py and the alignment tests: the cross-attention probabilities of the fp32 oracle (oracle/dit.py),
captured around its `attention` function; the bound within which they reproduce the reference's maps in tests/golden/g18_alignment.npz (the
generator asserts it when it writes the fixture, tests/test_align_cpu.py checks the tiny case against it on every CPU run); and the seeded
inputs of the fixture, which it pins by checksums instead of storing them (the full case's encoder states alone are 1.7 MB)."""
import contextlib

import torch

G18_ORACLE_BOUND = 1e-5   # max |oracle - reference| over the stored probabilities
G18_STEPS = 8             # inference_steps of the fixture's rows: t = 1 / 8


def g18_inputs(T, L, D, seed):
    """pred / noise / context / encoder states of one song, from CPU generators."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(1, T, 64, generator=g)
    noise = torch.randn(1, T, 64, generator=g)
    ctx = torch.cat([0.5 * torch.randn(1, T, 64, generator=g), torch.ones(1, T, 64)], -1)
    enc = torch.randn(1, L, D, generator=g)
    return pred, noise, ctx, enc


def g18_score_rows(pred, noise):
    """The score layout of get_lyric_score in fp32: [noise at t = 1 ; t noise + (1 - t) pred at t]."""
    t = 1.0 / G18_STEPS
    return torch.cat([noise, t * noise + (1 - t) * pred], 0), torch.tensor([1.0, t])


def checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


@contextlib.contextmanager
def capture_cross(o_dit):
    """Within the block, every `o_dit.dit_forward` appends layer l's cross-attention probabilities [N, Hq, S, L] (fp32, the softmax of
    eager_attention_forward; in bf16-storage mode from the bf16-rounded q / k, as the oracle's own contraction sees them) to the yielded
    list.  Each layer calls `attention` twice, self-attention first."""
    maps, calls, orig = [], [0], o_dit.attention

    def wrapped(q, k, v, mask, scale):
        if calls[0] % 2 == 1:
            kk = k.repeat_interleave(q.shape[1] // k.shape[1], dim=1)
            w = torch.matmul(o_dit._q(q), o_dit._q(kk).transpose(2, 3)) * scale
            maps.append(torch.softmax(w, dim=-1, dtype=torch.float32))
        calls[0] += 1
        return orig(q, k, v, mask, scale)
    o_dit.attention = wrapped
    try:
        yield maps
    finally:
        o_dit.attention = orig


def handler_layout(maps, prs):
    """[n_pairs, N, L, S]: layer l, head h of the captured [N, H, S, L] maps, transposed as the handlers transpose them."""
    return torch.stack([maps[l][:, h].transpose(-1, -2) for l, h in prs])
