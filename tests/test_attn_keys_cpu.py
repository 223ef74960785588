"""CPU: the method of tests/test_attention_keys_gpu.py, proven without a GPU.  A torch emulation of attn.hip's arithmetic (_attn_keys.emulate:
64-key tiles, a stale running max, p rounded to bf16, l in fp32, a bf16 quotient) goes through the same one-hot V, decoder and comparison
as the kernels and passes; the same emulation with one deliberate error - a band edge moved by one key, a pad key let in, the last key
counted twice, the wrong KV head, V read transposed, truncation for rounding - does not."""
import pytest
import torch

import _attn_keys as keys

# (N, Sq, Skv, Hq, Hkv, window), lens: ragged blocks and tiles, more than one 128-key run, Hq = 2 Hkv = 4 (h // 2 != h % Hkv)
FULL = ((2, 70, 130, 4, 2, -1), None)
BANDED = ((1, 200, 200, 2, 1, 16), None)
MASKED = ((3, 100, 100, 2, 1, 16), (100, 37, 0))   # an empty sequence; sequence 1's queries past 53 see no key


def _run(case, **errors):
    shape, lens = case
    return keys.run_case(shape, lens, lambda q, k, v: keys.emulate(q, k, v, shape, lens, **errors), seed=5, label=str(shape))


@pytest.mark.parametrize("case", [FULL, BANDED, MASKED], ids=["full", "banded", "masked"])
def test_the_emulated_kernel_passes(case):
    res = _run(case)
    print(f"{case[0]}: {res['runs']} runs, max error {res['max_err_u']:.3f} U, smallest visible p {res['min_p']:.3g}")
    assert res["min_p"] > keys.P_FLOOR
    assert res["n_bad"] == 0, res["report"]
    assert 0.0 < res["max_err_u"] <= keys.REL_BOUND / keys.U


def test_the_spike_moves_the_running_max_late():
    """The spike's score is far above every other key of its row and sits in a later tile than the row's first visible key."""
    for shape, lens in (FULL, BANDED, MASKED):
        q, k, (n, h, i, j) = keys.make_qk(shape, 5, lens)
        P, vis = keys.reference(q, k, shape, lens, [(n, h)])
        assert vis[0, i, j] and (j == shape[2] - 1 or not vis[0, i, j + 1]) and P[0, i, j] > 0.99
        assert j // 64 > int(vis[0, i].nonzero()[0]) // 64


@pytest.mark.parametrize("case,errors", [
    (BANDED, dict(band_delta=-1)), (BANDED, dict(band_delta=1)), (FULL, dict(pad_leak=True)), (FULL, dict(double_last=True)),
    (FULL, dict(kv_head_mod=True)), (FULL, dict(v_transposed=True)), (FULL, dict(truncate=True)), (BANDED, dict(truncate=True)),
    (MASKED, dict(band_delta=-1)), (MASKED, dict(band_delta=1)),
], ids=["band-narrowed", "band-widened", "pad-key-let-in", "last-key-twice", "kv-head-mod", "v-transposed", "truncation", "truncation-banded",
        "masked-band-narrowed", "masked-band-widened"])
def test_a_deliberate_error_is_caught(case, errors):
    res = _run(case, **errors)
    print(res["report"])
    assert res["n_bad"] > 0


def test_one_hot_v_and_decode_round_trip():
    """decode inverts one_hot_v: out = P V with an exact P gives P back, strays are zero, and perm is a permutation but no involution."""
    x = torch.arange(128)
    assert sorted(keys.perm(x).tolist()) == list(range(128)) and not torch.equal(keys.perm(keys.perm(x)), x)
    shape = (3, 5, 130, 4, 2, -1)
    N, Sq, Skv, Hq, Hkv, _w = shape
    P = torch.rand(N, Hq, Sq, Skv).to(torch.bfloat16).float()
    for r in range(keys.n_runs(Skv)):
        v = keys.one_hot_v(shape, r).float().view(N, Skv, Hkv, 128)
        assert int((v != 0).sum()) == N * Hkv * min(128, Skv - 128 * r)
        out = torch.einsum("nhij,njhd->nihd", P, v.repeat_interleave(Hq // Hkv, dim=2)).reshape(N, Sq, Hq * 128).to(torch.bfloat16)
        got, stray = keys.decode(out, shape, r)
        assert torch.equal(got, P[..., 128 * r:128 * r + 128]) and not stray.any()
