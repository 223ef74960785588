"""CPU: the 5 Hz LM forward's fixture, oracle composition, configuration parsing, mask parser, decode plan, call contract and seam, with no
GPU (a fake stands in for the native handle)."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import _drift
import _lm_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_SYMBOLS = ("ace355_lm_create", "ace355_lm_destroy", "ace355_lm_load_tensor", "ace355_lm_finalize", "ace355_lm_prefill",
              "ace355_lm_decode", "ace355_lm_length", "ace355_lm_decode_plan")


# ------------------------------------------------------------------ G21
def test_g21_oracle_recompute_and_recorded_drift():
    from ace355 import weightgen
    z = L.load_g21()
    assert os.path.getsize(L.G21) <= 1 << 20
    w = L.weights("wide")
    assert abs(weightgen.checksum(w) - float(z["wide_checksum"])) <= 1e-9 * float(z["wide_checksum"])
    ids, first, P = torch.from_numpy(z["wide_ids"]).long(), [int(v) for v in z["wide_first"]], int(z["wide_P"])
    assert ids.shape == (3, P + 4) and first == [0, 5, P - 1] and z["wide_logits"].shape == (5, 3, L.WIDE.vocab_size)
    ref = torch.from_numpy(z["wide_logits"])
    for t, out in enumerate(L.teacher_forced(L.WIDE, w, ids, first, P)):
        assert L.rel(out, ref[t]) <= L.G21_ORACLE_BOUND, f"step {t}"
    # the recorded drift is this oracle's bf16-storage mode (recomputed for the prefill and the last step)
    for t in (0, 4):
        emu = _drift.emulated(L.lm_logits, L.WIDE, w, ids[:, :P + t], first)
        assert abs(L.rel(emu, ref[t]) - float(z["wide_drift_all"][t])) <= 1e-3 * float(z["wide_drift_all"][t])
    assert np.all(z["wide_drift"] > 0) and z["wide_drift"].shape == (5, 3)


def test_g21_seam_seed_qualifies_on_all_steps():
    """What make_g21_lm.py chose the token seed for: the bf16-storage emulation alone picks the oracle's greedy tokens on all 8 steps."""
    from ace355 import weightgen
    z = L.load_g21()
    w = L.weights("tiny")
    assert abs(weightgen.checksum(w) - float(z["tiny_checksum"])) <= 1e-9 * float(z["tiny_checksum"])
    ids, first, P = torch.from_numpy(z["seam_ids"]).long(), [int(v) for v in z["seam_first"]], int(z["seam_P"])
    assert ids.shape == (2, P + 8) and first[0] == 0 and 0 < first[1] < P
    for t in range(8):
        ref = L.lm_logits(L.TINY, w, ids[:, :P + t], first)
        emu = _drift.emulated(L.lm_logits, L.TINY, w, ids[:, :P + t], first)
        top2 = ref.topk(2, dim=-1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > 4.0 * float((emu - ref).abs().max()), t
        assert torch.equal(ref.argmax(-1), ids[:, P + t]) and torch.equal(emu.argmax(-1), ids[:, P + t]), t


def test_composition_hides_pads_and_needs_no_cache():
    """The oracle composition the gates rest on: ids below first[n] are invisible, a visible id is not, sequences are independent."""
    w = L.weights("tiny")
    ids, first = L.left_padded((12, 7, 1), 12, L.TINY.vocab_size, 3)
    a = L.lm_logits(L.TINY, w, ids, first)
    assert torch.isfinite(a).all()
    b_ids = ids.clone()
    b_ids[1, :5] = 77
    b_ids[2, :11] = 78
    assert torch.equal(L.lm_logits(L.TINY, w, b_ids, first), a)
    c_ids = ids.clone()
    c_ids[1, 5] = (c_ids[1, 5] + 1) % L.TINY.vocab_size
    c = L.lm_logits(L.TINY, w, c_ids, first)
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and not torch.equal(c[1], a[1])
    # an unpadded row equals the same row run alone
    assert torch.allclose(L.lm_logits(L.TINY, w, ids[:1], first[:1]), a[:1], rtol=0, atol=1e-5)
    # one causal pass over the whole length gives every step's logits: the full recompute the GPU tests compare decode steps against
    more = torch.cat([ids, torch.randint(0, L.TINY.vocab_size, (3, 4), generator=torch.Generator().manual_seed(4))], 1)
    every = L.lm_logits_at(L.TINY, w, more, first, range(11, 16))
    for t, step in enumerate(L.teacher_forced(L.TINY, w, more, first, 12)):
        assert L.rel(every[:, t], step) <= L.G21_ORACLE_BOUND
    untied = L.weights("tiny_untied")
    assert "lm_head.weight" in untied and "lm_head.weight" not in w


# ------------------------------------------------------------------ configuration
def _qwen3_like(**over):
    base = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                vocab_size=1003, rms_norm_eps=1e-6, use_sliding_window=False, attention_bias=False, rope_theta=1e6,
                layer_types=["full_attention", "full_attention"], tie_word_embeddings=True)
    base.update(over)
    return types.SimpleNamespace(**base)


def test_config_from_reference():
    from ace355.config import LmConfig
    assert LmConfig.from_reference(_qwen3_like()) == L.TINY
    assert LmConfig.from_reference(_qwen3_like(tie_word_embeddings=False)) == L.TINY_UNTIED
    new = LmConfig.from_reference(_qwen3_like(rope_theta=None, rope_parameters={"rope_type": "default", "rope_theta": 5e5}))
    assert new.rope_theta == 5e5
    shapes = L.WIDE.weight_shapes()
    assert shapes["model.embed_tokens.weight"] == (2051, 512) and shapes["lm_head.weight"] == (2051, 512)
    assert shapes["model.layers.1.self_attn.q_proj.weight"] == (2048, 512) and shapes["model.norm.weight"] == (512,)
    assert len(shapes) == 3 + 2 * 11 and len(L.TINY.weight_shapes()) == 2 + 2 * 11


@pytest.mark.parametrize("over", [dict(use_sliding_window=True), dict(layer_types=["full_attention", "sliding_attention"]),
                                  dict(attention_bias=True), dict(rope_scaling={"rope_type": "yarn", "factor": 2.0}),
                                  dict(rope_parameters={"rope_type": "linear", "rope_theta": 1e6, "factor": 2.0}),
                                  dict(num_attention_heads=32, num_key_value_heads=8),   # Qwen3-4B
                                  dict(num_attention_heads=4, num_key_value_heads=4), dict(head_dim=64)])
def test_config_refusals(over):
    from ace355.config import LmConfig
    with pytest.raises(NotImplementedError):
        LmConfig.from_reference(_qwen3_like(**over))


def test_config_struct_layout_matches_header(tmp_path):
    from ace355 import native
    ct = native.LmConfigC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_lm_config));',
             '  printf("limits %d %d %d\\n", ACE355_LM_MAX_SEQS, ACE355_LM_MAX_POSITIONS, ACE355_LM_MAX_TOKENS);']
    lines += [f'  printf("{f} %zu\\n", offsetof(ace355_lm_config, {f}));' for f, _t in ct._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(got["size"][0]) == ctypes.sizeof(ct) == 48
    assert [int(v) for v in got["limits"]] == [native.LM_MAX_SEQS, native.LM_MAX_POSITIONS, native.LM_MAX_TOKENS]
    for f, _t in ct._fields_:
        assert int(got[f][0]) == getattr(ct, f).offset, f


def test_lm_symbols_in_header_and_library():
    from ace355 import native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ace355.h")).read(), flags=re.S)
    lib = native.lib()
    for s in LM_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", src), f"{s} not declared in include/ace355.h"
        assert hasattr(lib, s) and s in native.SIGNATURES, s


# ------------------------------------------------------------------ the mask parser
def test_mask_parser_yields_first():
    from ace355.lm import left_pad_first
    m = torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]])
    assert left_pad_first(m) == [0, 2, 3]
    assert left_pad_first(m.bool()) == [0, 2, 3] and left_pad_first(m.float()) == [0, 2, 3]


@pytest.mark.parametrize("rows", [[[1, 0, 1, 1]], [[0, 1, 0, 1]],          # holes
                                  [[1, 1, 1, 0]], [[0, 1, 1, 0]],          # right pads
                                  [[1, 1, 1, 1], [0, 0, 0, 0]]])           # an all-zero row
def test_mask_parser_refusals(rows):
    from ace355.lm import left_pad_first
    with pytest.raises(NotImplementedError):
        left_pad_first(torch.tensor(rows))


# ------------------------------------------------------------------ the decode plan
def test_plan_sweep_under_host_sanitizers(tmp_path):
    """csrc/lm_plan.h as a host program: for every length 1 .. 4100 the chunks tile [0, len) exactly once, in order; the regimes it
    prints are the ones the library answers with, and the library's answer depends on the length only (it takes nothing else)."""
    from ace355 import native
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "lm_plan_sweep"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "lm_plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "4100"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert "ok 4100" in lines
    regimes = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("regime")]
    assert regimes == [(1, 64, 1), (257, 128, 3), (1025, 256, 5)], regimes
    for start, chunk, splits in regimes:
        assert native.lm_decode_plan(start) == {"chunk": chunk, "splits": splits}
        if start > 1:
            assert native.lm_decode_plan(start - 1)["chunk"] != chunk
    for length in (1, 64, 65, 256, 1024, 4096, native.LM_MAX_POSITIONS):
        p = native.lm_decode_plan(length)
        assert p["splits"] == -(-length // p["chunk"]) <= 64
    for bad in (0, -1, native.LM_MAX_POSITIONS + 1):
        assert native.lib().ace355_lm_decode_plan(bad, ctypes.byref(ctypes.c_int32()), ctypes.byref(ctypes.c_int32())) == 1


# ------------------------------------------------------------------ call contract (fake native handle)
def _fake_lm(cfg=L.TINY, out_dtype=torch.float32, max_positions=64):
    from ace355.lm import NativeCausalLM

    class Fake(NativeCausalLM):
        def __init__(self):
            self.cfg, self.device, self.out_dtype = cfg, torch.device("cpu"), out_dtype
            self.max_positions, self.max_seqs = max_positions, 16
            self._generation, self._first, self.len = 0, None, 0
            self.calls = []

        def _prefill(self, ids, first, out):
            assert ids.dtype == torch.int32 and ids.is_contiguous() and first.dtype == torch.int32
            self.calls.append(("prefill", ids.clone(), first.tolist()))
            self.len = ids.shape[1]
            out.copy_(torch.nn.functional.one_hot(ids[:, -1].long(), cfg.vocab_size).float())

        def _decode(self, ids, out):
            self.calls.append(("decode", ids.clone()))
            self.len += 1
            out.copy_(torch.nn.functional.one_hot(ids.long(), cfg.vocab_size).float())

        def _length(self):
            return self.len

        def close(self):
            pass

    return Fake()


def test_call_contract_follows_forward_pass():
    lm = _fake_lm()
    ids, first = L.left_padded((9, 4), 9, L.TINY.vocab_size, 1)
    mask = L.mask_of(first, 9)
    o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
    assert o.logits.shape == (2, 1, L.TINY.vocab_size) and o.logits.dtype == torch.float32 and lm.length == 9
    assert torch.equal(o.logits[:, -1, :].argmax(-1), ids[:, -1]) and lm.calls[-1][2] == [0, 5]
    past = o.past_key_values
    for t in range(1, 4):
        nxt = torch.tensor([[t], [t + 10]])
        mask = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1)
        o = lm(input_ids=nxt, past_key_values=past, attention_mask=mask, use_cache=True)
        past = o.past_key_values
        assert lm.calls[-1][0] == "decode" and lm.calls[-1][1].tolist() == [t, t + 10] and lm.length == 9 + t
        assert o.logits.shape == (2, 1, L.TINY.vocab_size)
    assert lm.prefill(ids).shape == (2, L.TINY.vocab_size) and lm.calls[-1][2] == [0, 0] and lm.length == 9
    assert lm.decode(torch.tensor([3, 4])).shape == (2, L.TINY.vocab_size)
    assert _fake_lm(out_dtype=torch.bfloat16)(ids, mask[:, :9]).logits.dtype == torch.bfloat16


def _started():
    lm = _fake_lm()
    ids, first = L.left_padded((6, 3), 6, L.TINY.vocab_size, 2)
    mask = L.mask_of(first, 6)
    o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
    return lm, ids, mask, o.past_key_values


@pytest.mark.parametrize("case", ["stale_token", "foreign_token", "hf_cache", "mask_width", "mask_padding", "mask_holes", "ids_shape",
                                  "position_ids", "inputs_embeds", "labels", "hidden_states", "attentions", "logits_to_keep", "unknown"])
def test_unsupported_calls_raise_before_any_native_call(case):
    lm, ids, mask, past = _started()
    n_calls = len(lm.calls)
    one = torch.ones(2, 1, dtype=mask.dtype)
    nxt, mask7 = torch.tensor([[1], [2]]), torch.cat([mask, one], 1)
    kw = dict(input_ids=nxt, past_key_values=past, attention_mask=mask7, use_cache=True)
    if case == "stale_token":
        lm(**kw)                         # consumes `past`
        n_calls += 1
        kw["attention_mask"] = torch.cat([mask7, one], 1)
    elif case == "foreign_token":
        kw["past_key_values"] = _started()[3]
    elif case == "hf_cache":
        kw["past_key_values"] = object()
    elif case == "mask_width":
        kw["attention_mask"] = mask
    elif case == "mask_padding":
        kw["attention_mask"] = torch.ones_like(mask7)
    elif case == "mask_holes":
        kw = dict(input_ids=ids, attention_mask=torch.tensor([[1, 1, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1]]))
    elif case == "ids_shape":
        kw["input_ids"] = torch.tensor([[1, 2], [3, 4]])
    elif case == "position_ids":
        kw["position_ids"] = torch.zeros(2, 1, dtype=torch.long)
    elif case == "inputs_embeds":
        kw["inputs_embeds"] = torch.zeros(2, 1, 256)
    elif case == "labels":
        kw["labels"] = nxt
    elif case == "hidden_states":
        kw["output_hidden_states"] = True
    elif case == "attentions":
        kw["output_attentions"] = True
    elif case == "logits_to_keep":
        kw["logits_to_keep"] = 3
    else:
        kw["something_else"] = 1
    with pytest.raises(NotImplementedError):
        lm(**kw)
    assert len(lm.calls) == n_calls


@pytest.mark.parametrize("bad", [-1, L.TINY.vocab_size])
def test_out_of_range_ids_and_full_cache_raise_before_native(bad):
    lm, ids, mask, past = _started()
    n_calls = len(lm.calls)
    with pytest.raises(ValueError):
        lm(input_ids=torch.tensor([[1], [bad]]), past_key_values=past, attention_mask=torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1))
    ids2 = ids.clone()
    ids2[0, 1] = bad
    with pytest.raises(ValueError):
        lm.prefill(ids2)
    small = _fake_lm(max_positions=6)
    small.prefill(ids)
    with pytest.raises(ValueError):
        small.decode(torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        small.prefill(torch.zeros(2, 7, dtype=torch.long))
    with pytest.raises(ValueError):
        _fake_lm().decode(torch.tensor([1, 2]))
    assert len(lm.calls) == n_calls and len(small.calls) == 1
    # the refused calls left the token usable
    lm(input_ids=torch.tensor([[1], [2]]), past_key_values=past, attention_mask=torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype)], 1))


# ------------------------------------------------------------------ seam
class _RefLm(torch.nn.Module):
    """Stands in for the reference Qwen3ForCausalLM: records its calls and returns a cache object of its own."""

    def __init__(self):
        super().__init__()
        self.lm_head = torch.nn.Linear(4, 4)
        self.config = types.SimpleNamespace(name="ref-config")
        self.calls = []

    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, **kw):
        self.calls.append((tuple(input_ids.shape), past_key_values))
        cache = past_key_values if past_key_values is not None else ["ref-cache"]
        return types.SimpleNamespace(logits=torch.zeros(input_ids.shape[0], input_ids.shape[1], 4), past_key_values=cache)

    def generate(self, *a, **k):
        return "ref-generate"


def test_swap_routes_by_cache_object():
    from ace355.modswap import NativeCausalLMSwap
    ref, fake = _RefLm(), _fake_lm()
    sw = NativeCausalLMSwap(fake, ref, "llm")
    assert list(sw.state_dict().keys()) == list(ref.state_dict().keys())
    assert sw.generate() == "ref-generate" and sw.config is ref.config
    ids, first = L.left_padded((6, 3), 6, L.TINY.vocab_size, 2)
    mask, one = L.mask_of(first, 6), torch.ones(2, 1, dtype=torch.long)
    # a good generation never reaches the kept module
    o = sw(input_ids=ids, attention_mask=mask, use_cache=True)
    mask7 = torch.cat([mask, one], 1)
    o = sw(input_ids=ids[:, -1:], past_key_values=o.past_key_values, attention_mask=mask7, use_cache=True)
    assert ref.calls == [] and sw.native_calls == 2 and [c[0] for c in fake.calls] == ["prefill", "decode"]
    # a holed mask goes to the kept module, and so does the step that carries the kept module's cache
    holes = mask.clone()
    holes[0, 2] = 0
    r = sw(input_ids=ids, attention_mask=holes, use_cache=True)
    assert r.past_key_values == ["ref-cache"] and sw.native_failures == 1 and len(ref.calls) == 1
    r2 = sw(input_ids=ids[:, -1:], past_key_values=r.past_key_values, attention_mask=torch.cat([holes, one], 1), use_cache=True)
    assert r2.past_key_values is r.past_key_values and len(ref.calls) == 2 and ref.calls[1][1] is r.past_key_values
    assert len(fake.calls) == 2 and sw.native_calls == 2
    # an error inside a native decode step propagates
    o = sw(input_ids=ids, attention_mask=mask, use_cache=True)
    with pytest.raises(NotImplementedError):
        sw(input_ids=ids[:, -1:], past_key_values=o.past_key_values, attention_mask=mask, use_cache=True)   # wrong width
    assert len(ref.calls) == 2


def test_init_native_lm_refusals_and_never_raises(monkeypatch):
    from ace355 import modswap
    from ace355.backend import NativeLmMixin

    class Host(NativeLmMixin):
        pass

    for offload, dev in ((True, "cuda:0"), (False, "cpu")):
        h = Host()
        h.llm, h.device, h.offload_to_cpu = _RefLm(), dev, offload
        before = h.llm
        assert h._init_native_lm() is False and h.llm is before and h.use_native_lm is False
    h = Host()
    h.llm, h.device, h.offload_to_cpu = _RefLm(), "cuda:0", False
    before = h.llm

    def boom(*a, **k):
        raise RuntimeError("no library")
    monkeypatch.setattr(modswap, "swap_in_lm", boom)
    assert h._init_native_lm() is False and h.llm is before
    h.llm = None
    assert h._init_native_lm() is False
