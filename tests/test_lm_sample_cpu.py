"""CPU: the LM token selection's fixture against its fp64 restatement, the ABI struct, the pure plan and workspace functions, the
refusals of ``ace355_lm_pick`` (all made before any HIP call) and the seam's pass-through, with no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _lm_sample_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_V = 217205


# ------------------------------------------------------------------ G22
def test_g22_oracle_equals_reference_on_every_case():
    assert os.path.getsize(O.G22) <= 1 << 20
    cases = O.load_g22()
    assert [c[0].shape for c in cases[:7]] == [(3, V) for V in (1, 2, 63, 64, 65, 1003, 2051)] and len(cases) == 12
    margin = float(np.load(O.G22)["margin"])
    assert margin == 1e-3
    rows = 0
    for x, sets in cases:
        assert len(sets) == O.SETTINGS
        for k, p, fin, greedy in sets:
            for r in range(x.shape[0]):
                keep = O.keep_mask(x[r], k, p)
                assert np.array_equal(keep, fin[r]), (x.shape, k, p, r)
                assert O.greedy_token(x[r], keep) == int(greedy[r])
                dist, differ = O.top_p_margin(x[r], k, p)
                assert dist >= margin and differ
                rows += 1
    assert rows == (7 * 3 + 5) * 4


def test_g22_holds_the_edge_rows():
    cases = O.load_g22()
    codes, eos, dup, peaked, few = (c[0][0] for c in cases[7:])
    fin = np.isfinite(codes)
    assert fin[300:900].all() and fin[2000] and fin.sum() == 601
    assert np.isfinite(eos).sum() == 1
    kth = np.sort(dup)[::-1][49]
    assert (dup == kth).sum() == 5 and cases[9][1][1][2][0].sum() == 54     # every tie at the k-th value survives
    assert cases[10][1][0][2][0].sum() == 1                                  # the peaked row keeps one entry under p = 0.9
    assert np.isfinite(few).sum() == 20 and cases[11][1][1][0] == 50 and cases[11][1][1][2][0].sum() == 20


def test_oracle_rules():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 3.0], dtype=np.float32)
    assert O.keep_mask(x, 2, None).tolist() == [False, True, True, False, False, True]      # ties at the k-th value survive
    assert O.keep_mask(x, 5, None).tolist() == [True, True, True, False, True, True]        # -inf is never kept
    # equal values in ascending id: masses 1, 1, 1 of Z = 3 + e^-1 + e^-2; position 2 has 2 / Z = 0.57 before it
    assert O.keep_mask(x, None, 0.5).tolist() == [False, True, True, False, False, False]
    assert O.keep_mask(x, None, 0.2).tolist() == [False, True, False, False, False, False]  # position 0 is always kept
    keep = O.keep_mask(x, None, None)
    assert O.greedy_token(x, keep) == 1
    assert O.token_for_u(x, keep, 1.0, 0.0) == 0 and O.token_for_u(x, keep, 1.0, np.nextafter(np.float32(1), np.float32(0))) == 5
    for bad in ([1.0, np.nan], [1.0, np.inf], [-np.inf, -np.inf]):
        assert O.is_bad(bad) and not O.keep_mask(bad).any() and O.token_for_u(bad, O.keep_mask(bad), 1.0, 0.5) == -1
    z = np.array([-0.0, 0.0, -1.0], dtype=np.float32)
    assert O.keep_mask(z, 1, None).tolist() == [True, True, False]                          # -0.0 == +0.0


# ------------------------------------------------------------------ ABI
def test_pick_params_layout_matches_header(tmp_path):
    from ace355 import native
    ct = native.LmPickParamsC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_lm_pick_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ace355_lm_pick_params, {f}));' for f, _t in ct._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 16
    assert [f for f, _t in ct._fields_] == ["top_k", "top_p", "temperature", "reserved"]
    for f, _t in ct._fields_:
        assert int(got[f]) == getattr(ct, f).offset, f


def test_plan_is_a_pure_cut_of_the_row():
    from ace355 import native
    lib = native.lib()
    prev = 0
    for V in list(range(1, 4101)) + [8191, 8192, 8193, 16384, 16385, REAL_V, native.LM_PICK_MAX_V]:
        p = native.lm_pick_plan(V)
        assert p == native.lm_pick_plan(V)
        chunk, chunks = p["chunk"], p["chunks"]
        assert chunk > 0 and chunks == -(-V // chunk) >= 1
        # chunk c = [c * chunk, min(V, (c + 1) * chunk)): every id once, in order, no empty chunk
        edges = [(c * chunk, min(V, (c + 1) * chunk)) for c in range(chunks)]
        assert edges[0][0] == 0 and edges[-1][1] == V and all(lo < hi for lo, hi in edges)
        assert all(edges[i][1] == edges[i + 1][0] for i in range(chunks - 1))
        assert chunks >= prev
        prev = chunks
    assert native.lm_pick_plan(REAL_V)["chunks"] == 27
    for bad in (0, -1, native.LM_PICK_MAX_V + 1):
        assert lib.ace355_lm_pick_plan(bad, ctypes.byref(ctypes.c_int32()), ctypes.byref(ctypes.c_int32())) == 1
        assert "lm_pick_plan" in native.last_error()
    assert lib.ace355_lm_pick_plan(5, None, None) == 1


def test_workspace_bytes_is_pure_and_monotone():
    from ace355 import native
    f = native.lib().ace355_lm_pick_workspace_bytes
    for V in (1, 64, 8192, 8193, REAL_V):
        sizes = [f(B, V) for B in range(1, native.LM_MAX_SEQS + 1)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        assert sizes == [f(B, V) for B in range(1, native.LM_MAX_SEQS + 1)]
    by_v = [f(3, V) for V in (1, 100, 8192, 8193, 100000, REAL_V, native.LM_PICK_MAX_V)]
    assert by_v == sorted(by_v) and f(3, 8193) > f(3, 8192)
    assert f(16, REAL_V) < 32 << 20
    for B, V in ((0, 100), (-1, 100), (native.LM_MAX_SEQS + 1, 100), (1, 0), (1, -5), (1, native.LM_PICK_MAX_V + 1)):
        assert f(B, V) == 0


@pytest.mark.parametrize("case", ["B_zero", "B_large", "V_zero", "V_large", "stride", "null_logits", "null_params", "null_tokens",
                                  "null_workspace", "null_u", "small_workspace"])
def test_pick_refusals_need_no_gpu(case):
    """Each defect alone is refused with ACE355_ERR_INVALID and a message before any HIP call: the pointers here are not memory."""
    from ace355 import native
    lib = native.lib()
    B, V = 2, 100
    need = lib.ace355_lm_pick_workspace_bytes(B, V)
    a = dict(logits=4096, stride=V, B=B, V=V, params=native.LmPickParamsC(0, 0.9, 0.85, 0), u=4096, tokens=4096, kept=None, keep=None,
             ws=4096, ws_bytes=need)
    word = {"B_zero": "B must", "B_large": "B must", "V_zero": "V must", "V_large": "V must", "stride": "row_stride",
            "null_logits": "null", "null_params": "null", "null_tokens": "null", "null_workspace": "null", "null_u": "u is required",
            "small_workspace": "workspace"}[case]
    if case == "B_zero":
        a["B"] = 0
    elif case == "B_large":
        a["B"] = native.LM_MAX_SEQS + 1
    elif case == "V_zero":
        a["V"] = 0
    elif case == "V_large":
        a["V"], a["stride"] = native.LM_PICK_MAX_V + 1, native.LM_PICK_MAX_V + 1
    elif case == "stride":
        a["stride"] = V - 1
    elif case == "null_logits":
        a["logits"] = None
    elif case == "null_params":
        a["params"] = None
    elif case == "null_tokens":
        a["tokens"] = None
    elif case == "null_workspace":
        a["ws"] = None
    elif case == "null_u":
        a["u"] = None
    else:
        a["ws_bytes"] = need - 1
    lib.ace355_lm_pick_plan(0, None, None)   # leaves another message behind
    par = ctypes.byref(a["params"]) if a["params"] is not None else None
    rc = lib.ace355_lm_pick(a["logits"], a["stride"], a["B"], a["V"], par, a["u"], a["tokens"], a["kept"], a["keep"], a["ws"],
                            a["ws_bytes"], None)
    assert rc == 1 and "lm_pick:" in native.last_error() and word in native.last_error(), native.last_error()


# ------------------------------------------------------------------ the seam, where it must not change anything
class _Base:
    """Restates the three reference methods (llm_inference.py:367-399) and counts its calls."""

    def __init__(self):
        self.calls = []

    def _apply_top_k_filter(self, logits, top_k):
        self.calls.append("k")
        if top_k is not None and top_k > 0:
            logits[logits < torch.topk(logits, top_k)[0][..., -1, None]] = float("-inf")
        return logits

    def _apply_top_p_filter(self, logits, top_p):
        self.calls.append("p")
        if top_p is not None and 0.0 < top_p < 1.0:
            s, idx = torch.sort(logits, descending=True)
            rem = torch.cumsum(torch.softmax(s.float(), dim=-1), dim=-1) > top_p
            rem[..., 1:] = rem[..., :-1].clone()
            rem[..., 0] = 0
            logits[rem.scatter(1, idx, rem)] = float("-inf")
        return logits

    def _sample_tokens(self, logits, temperature):
        self.calls.append("s")
        if temperature > 0:
            return torch.multinomial(torch.softmax(logits.float() / temperature, dim=-1), num_samples=1).squeeze(1)
        return torch.argmax(logits, dim=-1)


def _handler(flag):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _Base):
        pass

    h = Handler()
    if flag is not None:
        h.use_native_lm_sampler = flag
    return h


@pytest.mark.parametrize("flag", [None, False, True])
def test_seam_passes_through_when_off_or_on_cpu(flag, monkeypatch):
    """Flag off (the default without ACE355_LM_SAMPLER=1), or on with a CPU tensor: the base methods run, in place, and the native
    module is never asked."""
    from ace355 import backend, lmsample
    if flag is None:
        assert backend.NativeLmMixin.use_native_lm_sampler is (os.environ.get("ACE355_LM_SAMPLER", "") == "1")
        flag = False

    def boom(*a, **k):
        raise AssertionError("the native selection must not be called")
    monkeypatch.setattr(lmsample, "select_tokens", boom)
    x0 = torch.randn(3, 65, generator=torch.Generator().manual_seed(5)) * 3
    h, ref = _handler(flag), _Base()
    x, y = x0.clone(), x0.clone()
    for obj, t in ((h, x), (ref, y)):
        out = obj._apply_top_k_filter(t, 20)
        assert out is t
        out = obj._apply_top_p_filter(out, 0.9)
        assert out is t
    assert torch.equal(x, y) and torch.isinf(x).any()
    assert torch.equal(h._sample_tokens(x, 0.0), ref._sample_tokens(y, 0.0))
    torch.manual_seed(3)
    a = h._sample_tokens(x, 0.85)
    torch.manual_seed(3)
    assert torch.equal(a, ref._sample_tokens(y, 0.85))
    assert h.calls == ["k", "p", "s", "s"] and h._lm_sampler_record is None
