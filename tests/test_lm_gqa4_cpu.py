"""CPU: the opt-in for four q heads per kv head (Qwen3-4B's 32 / 8 layout) through every host layer - configuration parsing, the C ABI's
``ace355_lm_create_ex``, the pass plan and the GEMM plan at the 4B's shape, the 2 : 1 plans against a record made before the change, the
seam (a stub stands in for the library), the plan sweep as a host program, and fixture G25 - with no GPU."""
import contextlib
import ctypes
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import _drift
import _lm_gqa4_oracle as Q
import _lm_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS_4B = (2560, 9728, 32, 8, 36)   # hidden, intermediate, heads, kv heads, layers


def _qwen3_like(**over):
    base = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                vocab_size=1003, rms_norm_eps=1e-6, use_sliding_window=False, attention_bias=False, rope_theta=1e6,
                layer_types=["full_attention", "full_attention"], tie_word_embeddings=True)
    base.update(over)
    return types.SimpleNamespace(**base)


# ------------------------------------------------------------------ configuration
def test_config_opt_in():
    from ace355.config import LmConfig
    assert LmConfig.from_reference(_qwen3_like(), allow_gqa4=True) == Q.GQA4_TINY
    big = LmConfig.from_reference(_qwen3_like(num_attention_heads=32, num_key_value_heads=8), allow_gqa4=True)
    assert (big.num_attention_heads, big.num_key_value_heads) == (32, 8)
    assert LmConfig.from_reference(_qwen3_like(num_attention_heads=4), allow_gqa4=True) == L.TINY   # 2 : 1 is served as ever
    for over in (dict(num_attention_heads=4, num_key_value_heads=4), dict(num_attention_heads=16, num_key_value_heads=2), dict(head_dim=64),
                 dict(use_sliding_window=True)):
        with pytest.raises(NotImplementedError):
            LmConfig.from_reference(_qwen3_like(**over), allow_gqa4=True)
    for kw in ({}, dict(allow_gqa4=False)):   # without the opt-in: today's refusal, with today's text
        with pytest.raises(NotImplementedError, match=r"LM head layout 8 / 2 heads of 128 \(only 2 q heads per kv head, head_dim 128\)"):
            LmConfig.from_reference(_qwen3_like(), **kw)


def test_weight_shapes_at_the_4b_dimensions():
    s = Q.LM_4B.weight_shapes()
    assert s["model.layers.35.self_attn.q_proj.weight"] == (4096, 2560) and s["model.layers.0.self_attn.k_proj.weight"] == (1024, 2560)
    assert s["model.layers.35.self_attn.o_proj.weight"] == (2560, 4096) and s["model.layers.35.mlp.down_proj.weight"] == (2560, 9728)
    assert s["model.embed_tokens.weight"] == (217205, 2560) and "lm_head.weight" not in s and len(s) == 2 + 36 * 11


# ------------------------------------------------------------------ the C ABI
def test_create_ex_in_header_library_and_signatures():
    from ace355 import native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ace355.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ace355_lm_create_ex\s*\(\s*const\s+ace355_lm_config\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*ace355_lm\s*\*\*\s*\w*\s*\)", src)
    m = re.search(r"#define\s+ACE355_LM_ALLOW_GQA4\s+(\w+)", src)
    assert m and int(m.group(1).rstrip("uU"), 0) == native.LM_ALLOW_GQA4 == 1
    assert hasattr(native.lib(), "ace355_lm_create_ex")
    restype, argtypes = native.SIGNATURES["ace355_lm_create_ex"]
    assert restype is ctypes.c_int and argtypes[1] is ctypes.c_uint32 and len(argtypes) == 3
    assert ctypes.sizeof(native.LmConfigC) == 48   # the struct did not grow: the flag travels beside it


# ------------------------------------------------------------------ plans
def test_pass_plan_at_the_4b_shape():
    from ace355 import native
    cache = dict(causal=1, has_cache=1, max_pos=4096, max_seqs=16, has_first=1)
    for N, S in ((2, 512), (16, 2048)):
        p = native.encoder_pass_plan(*DIMS_4B, N, S, pos0=0, **cache)
        assert p["n_steps"] == len(p["steps"]) == 36 * 8 + 1 and p["QKV"] == 6144 and p["M"] == N * S
        assert p["calls"]["causal_attn"] == p["calls"]["kv_store"] == 36 and p["calls"]["decode_attn"] == 0 and p["calls"]["gemm"] == 4 * 36
        attn = [s for s in p["steps"] if s["kind"] == "causal_attn"]
        assert all(s["Hkv"] == 8 and s["ld"] == 6144 and s["k_col0"] == 4096 and s["v_col0"] == 5120 and s["o_ld"] == 32 * 128 and s["seqs"] == N and
                   s["Sq"] == S and s["first"] == 1 for s in attn)
        o = [s for s in p["steps"] if s["kind"] == "gemm" and s["proj"] == "o"]
        assert all((s["N"], s["K"]) == (2560, 4096) for s in o) and len(o) == 36
    p = native.encoder_pass_plan(*DIMS_4B, 16, 1, pos0=1299, **cache)
    dec = [s for s in p["steps"] if s["kind"] == "decode_attn"]
    want = native.lm_decode_plan(1300)
    assert len(dec) == 36 and all(s["len"] == 1300 and s["chunk"] == want["chunk"] and s["splits"] == want["splits"] and s["Hkv"] == 8 and
                                  s["ld"] == 6144 for s in dec)
    for fields in (dict(causal=1), dict(pos0=0, **cache), dict(pos0=1299, **cache)):
        with pytest.raises(Exception, match="2 or 4 q heads per kv head"):
            native.encoder_pass_plan(2560, 9728, 40, 8, 36, 2, 1 if fields.get("pos0") else 512, **fields)


def test_two_to_one_plans_are_what_they_were():
    """tests/golden/lm_plan_2to1.json was recorded on the commit before the 4 : 1 layout (tests/golden/make_lm_plan_2to1.py)."""
    from ace355 import native
    path = os.path.join(ROOT, "tests", "golden", "lm_plan_2to1.json")
    assert os.path.getsize(path) <= 1 << 20
    rows = json.load(open(path))
    assert len(rows) >= 20 and all(r["request"][2] == 2 * r["request"][3] for r in rows)
    for r in rows:
        now = json.loads(json.dumps(native.encoder_pass_plan(*r["request"], **r["fields"])))
        assert now == r["plan"], (r["request"], r["fields"])


def test_gemm_plan_takes_the_4b_projections():
    from ace355 import native
    D, F, QD, QKV = 2560, 9728, 4096, 6144
    for M in (2, 16, 32768):
        for n, k, mode in ((QKV, D, 4), (D, QD, 2), (2 * F, D, 3), (D, F, 2)):
            p = native.gemm_plan(M, n, k, mode)
            assert isinstance(p, dict) and p, (M, n, k, mode)


# ------------------------------------------------------------------ the seam
class _StubLib:
    """Stands in for the library: records which create entry a constructor reached, refuses 4 : 1 unless asked as the library does."""

    def __init__(self):
        self.calls = []

    def _create(self, cfg, flags, out):
        c = cfg._obj
        ok = c.head_dim == 128 and (c.num_heads == 2 * c.num_kv_heads or (flags & 1 and c.num_heads == 4 * c.num_kv_heads))
        if ok:
            out._obj.value = 0x1000
        return 0 if ok else 4

    def ace355_lm_create(self, cfg, out):
        self.calls.append(("create", None))
        return self._create(cfg, 0, out)

    def ace355_lm_create_ex(self, cfg, flags, out):
        self.calls.append(("create_ex", int(flags)))
        return self._create(cfg, int(flags), out)

    def ace355_lm_destroy(self, h):
        self.calls.append(("destroy", None))


class _Ref4B(torch.nn.Module):
    def __init__(self, heads=32, kv=8):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.config = _qwen3_like(num_attention_heads=heads, num_key_value_heads=kv, hidden_size=768, intermediate_size=1216, vocab_size=2051,
                                  tie_word_embeddings=False)


@pytest.fixture
def stub(monkeypatch):
    from ace355 import native
    from ace355.lm import NativeCausalLM
    lib = _StubLib()
    loaded = []
    monkeypatch.setattr(native, "lib", lambda: lib)
    monkeypatch.setattr(native, "last_error", lambda: "lm_create: only head_dim 128 with num_heads == 2 * num_kv_heads is supported")
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(NativeCausalLM, "load_state_dict", lambda self, sd: loaded.append(len(sd)))
    lib.loaded = loaded
    return lib


def _host(llm, flag=None):
    from ace355.backend import NativeLmMixin

    class Host(NativeLmMixin):
        pass

    h = Host()
    if flag is not None:
        h.use_native_lm_gqa4 = flag
    h.llm, h.device, h.offload_to_cpu = llm, "cuda:0", False
    return h


def test_seam_keeps_the_module_without_the_flag(stub, caplog):
    from ace355.backend import NativeLmMixin
    assert NativeLmMixin.use_native_lm_gqa4 is (os.environ.get("ACE355_LM_GQA4", "") == "1")
    ref = _Ref4B()
    h = _host(ref, flag=False)
    assert h._init_native_lm() is False and h.llm is ref and h.use_native_lm is False
    assert stub.calls == [] and stub.loaded == []   # the configuration refused it before the library was asked
    assert "only 2 q heads per kv head" in caplog.text


def test_seam_passes_the_opt_in_down_to_create_ex(stub, caplog):
    import logging
    from ace355 import modswap, native
    caplog.set_level(logging.INFO)
    ref = _Ref4B()
    h = _host(ref, flag=True)
    assert h._init_native_lm() is True and h.use_native_lm is True
    assert isinstance(h.llm, modswap.NativeCausalLMSwap) and h.llm._reference is ref
    assert stub.calls == [("create_ex", native.LM_ALLOW_GQA4)] and stub.loaded == [1]
    lm = modswap.native_of(h.llm)
    assert (lm.cfg.num_attention_heads, lm.cfg.num_key_value_heads, lm.cfg.hidden_size) == (32, 8, 768)
    assert "32 / 8 heads" in caplog.text
    # a 2 : 1 host with the flag on is served too; one without the flag goes through the old entry
    stub.calls.clear()
    h2 = _host(_Ref4B(heads=16, kv=8), flag=True)
    assert h2._init_native_lm() is True and stub.calls == [("create_ex", 1)]
    stub.calls.clear()
    h3 = _host(_Ref4B(heads=16, kv=8), flag=False)
    assert h3._init_native_lm() is True and stub.calls == [("create", None)]
    # and the other ratios stay refused with the flag on
    stub.calls.clear()
    h4 = _host(_Ref4B(heads=64, kv=8), flag=True)
    assert h4._init_native_lm() is False and stub.calls == [] and not isinstance(h4.llm, modswap.NativeCausalLMSwap)


def test_constructor_refusal_is_not_implemented(stub):
    from ace355.config import LmConfig
    from ace355.lm import NativeCausalLM
    with pytest.raises(NotImplementedError):
        NativeCausalLM(Q.GQA4_TINY, "cuda:0", max_positions=16)
    assert stub.calls == [("create", None)]
    with pytest.raises(NotImplementedError):
        NativeCausalLM(LmConfig(**{**Q.GQA4_TINY.__dict__, "num_attention_heads": 16}), "cuda:0", max_positions=16, allow_gqa4=True)
    assert stub.calls[-1] == ("create_ex", 1)


# ------------------------------------------------------------------ the plan sweep, as a host program
def test_gqa4_plan_sweep_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "lm_gqa4_plan_sweep"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "lm_gqa4_plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"gqa4 pass plans: (\d+) planned \((\d+) steps\), (\d+) refused; failures: 0", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(3)) >= 17, r.stdout[-500:]


# ------------------------------------------------------------------ G25
def test_g25_oracle_recompute_and_recorded_drift():
    from ace355 import weightgen
    z = Q.load_g25()
    assert os.path.getsize(Q.G25) <= 1 << 20
    cfg, w = Q.GQA4_WIDE, Q.weights("gqa4_wide")
    assert abs(weightgen.checksum(w) - float(z["checksum"])) <= 1e-9 * float(z["checksum"])
    ids, first, P = torch.from_numpy(z["ids"]).long(), [int(v) for v in z["first"]], int(z["P"])
    assert ids.shape == (3, P + 4) and first == [0, 5, P - 1] and z["logits"].shape == (5, 3, cfg.vocab_size)
    ref = torch.from_numpy(z["logits"])
    with torch.no_grad():
        every = L.lm_logits_at(cfg, w, ids, first, range(P - 1, P + 4))
        for t in range(5):
            assert L.rel(every[:, t], ref[t]) <= L.G21_ORACLE_BOUND, f"step {t}"
        emu = _drift.emulated(L.lm_logits, cfg, w, ids[:, :P + 4], first)
    assert abs(L.rel(emu, ref[4]) - float(z["drift_all"][4])) <= 1e-3 * float(z["drift_all"][4])
    assert np.all(z["drift"] > 0) and z["drift"].shape == (5, 3)
