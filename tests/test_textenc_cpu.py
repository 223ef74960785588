"""CPU: the text encoder's fixture, configuration parsing, call contract and seam, with no GPU (a fake stands in for the native handle)."""
import ctypes
import logging
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _textenc_oracle as T


# ------------------------------------------------------------------ G19
def test_g19_tiny_checksum_and_oracle_recompute():
    from ace355 import weightgen
    z = T.load_g19()
    w = T.weights(T.TINY, T.TINY_SEED)
    assert abs(weightgen.checksum(w) - float(z["tiny_checksum"])) <= 1e-9 * float(z["tiny_checksum"])
    for case in ("tiny_a", "tiny_b"):
        ids = torch.from_numpy(z[f"{case}_ids"]).long()
        ref = torch.from_numpy(z[f"{case}_out"])
        out = T.text_encoder(T.TINY, w, ids)
        assert T.rel(out, ref) <= T.G19_ORACLE_BOUND, case
        for b in range(ids.shape[0]):
            assert abs(float(out[b].double().norm()) - float(z[f"{case}_norm"][b])) <= 1e-5 * float(z[f"{case}_norm"][b])
        assert np.all(z[f"{case}_drift"] > 0)


def test_g19_cases_and_files():
    z = T.load_g19()
    a = z["tiny_a_ids"]
    assert a.shape == (3, 37) and (a[1, 20:] == T.TINY_PAD).all() and (a[2, 1:] == T.TINY_PAD).all() and (a[:, 0] != T.TINY_PAD).all()
    assert z["tiny_b_ids"].shape == (2, 300)
    f = z["full_ids"]
    assert f.shape == (3, 256) and (f[1, 131:] == T.FULL_PAD).all() and (f[2, 7:] == T.FULL_PAD).all() and (f[0] != T.FULL_PAD).all()
    assert z["full_out"].shape == (3, 256, T.FULL.hidden_size) and z["full_drift"].shape == (3,)
    for p in [T.G19] + T.G19_FULL_PARTS:
        assert os.path.getsize(p) <= 1 << 20


def test_tiny_composition_is_causal_with_live_pad_rows():
    """The oracle composition the gates rest on: rows <= p ignore later tokens; pad rows are ordinary causal rows."""
    w = T.weights(T.TINY, T.TINY_SEED)
    ids = T.padded_ids((12, 5), 12, T.TINY.vocab_size, T.TINY_PAD, 3)
    out = T.text_encoder(T.TINY, w, ids)
    cut = T.text_encoder(T.TINY, w, ids[:, :8])
    assert torch.allclose(out[:, :8], cut, rtol=0, atol=1e-5)
    assert not torch.allclose(out[1, 5], out[1, 6])   # two pad rows at different positions differ


# ------------------------------------------------------------------ configuration
def _qwen3_like(**over):
    base = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                vocab_size=1003, rms_norm_eps=1e-6, use_sliding_window=False, attention_bias=False,
                layer_types=["full_attention", "full_attention"])
    base.update(over)
    return types.SimpleNamespace(**base)


def test_config_rope_theta_both_locations():
    from ace355.config import TextEncoderConfig
    old = TextEncoderConfig.from_reference(_qwen3_like(rope_theta=1e6, rope_scaling=None))
    new = TextEncoderConfig.from_reference(_qwen3_like(rope_parameters={"rope_type": "default", "rope_theta": 5e5}))
    assert old.rope_theta == 1e6 and new.rope_theta == 5e5
    assert old == T.TINY


@pytest.mark.parametrize("over", [dict(use_sliding_window=True), dict(layer_types=["full_attention", "sliding_attention"]),
                                  dict(attention_bias=True), dict(rope_theta=1e6, rope_scaling={"rope_type": "yarn", "factor": 2.0}),
                                  dict(rope_parameters={"rope_type": "linear", "rope_theta": 1e6, "factor": 2.0})])
def test_config_refusals(over):
    from ace355.config import TextEncoderConfig
    over.setdefault("rope_theta", 1e6)
    with pytest.raises(NotImplementedError):
        TextEncoderConfig.from_reference(_qwen3_like(**over))


def test_config_struct_layout_matches_header(tmp_path):
    from ace355 import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ct = native.TextEncConfigC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_textenc_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ace355_textenc_config, {f}));' for f, _t in ct._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 36
    for f, _t in ct._fields_:
        assert int(got[f]) == getattr(ct, f).offset, f


# ------------------------------------------------------------------ call contract (fake native handle)
def _fake_encoder(cfg=T.TINY, out_dtype=torch.bfloat16):
    from ace355.textenc import NativeTextEncoder

    class Fake(NativeTextEncoder):
        def __init__(self):
            self.cfg, self.device, self.out_dtype = cfg, torch.device("cpu"), out_dtype
            self.calls = []
            self.table = torch.randn(cfg.vocab_size, cfg.hidden_size, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)

        def _encode(self, ids, out):
            self.calls.append(("encode", ids.clone()))
            assert ids.dtype == torch.int32 and ids.is_contiguous()
            out.copy_(self.table[ids.long()].float().cumsum(1).to(torch.bfloat16))   # a causal stand-in

        def _embed(self, ids, out):
            self.calls.append(("embed", ids.clone()))
            out.view(-1, cfg.hidden_size).copy_(self.table[ids.long()])

        def close(self):
            pass

    return Fake()


def test_call_contract():
    te = _fake_encoder()
    ids = T.padded_ids((9, 4), 9, T.TINY.vocab_size, T.TINY_PAD, 1)
    a = te(ids)
    b = te(input_ids=ids, lyric_attention_mask=None)
    c = te(ids, torch.ones(2, 9, dtype=torch.long))
    assert a.last_hidden_state is a[0] and a[0].shape == (2, 9, T.TINY.hidden_size) and a[0].dtype == torch.bfloat16
    assert torch.equal(a[0], b.last_hidden_state) and torch.equal(a[0], c[0])
    assert [k for k, _ in te.calls] == ["encode"] * 3
    e = te.embed_tokens(torch.tensor([[0, T.TINY.vocab_size - 1, 5]]))
    assert e.shape == (1, 3, T.TINY.hidden_size) and torch.equal(e[0, 1], te.table[-1])
    assert _fake_encoder(out_dtype=torch.float32)(ids).last_hidden_state.dtype == torch.float32


@pytest.mark.parametrize("kw", [dict(attention_mask="holes"), dict(inputs_embeds=torch.zeros(1, 2, 256)),
                                dict(past_key_values=object()), dict(output_hidden_states=True), dict(output_attentions=True),
                                dict(something_else=1)])
def test_unsupported_arguments_raise(kw):
    te = _fake_encoder()
    ids = T.padded_ids((6, 6), 6, T.TINY.vocab_size, T.TINY_PAD, 2)
    if kw.get("attention_mask") == "holes":
        m = torch.ones(2, 6, dtype=torch.long)
        m[1, 4:] = 0
        kw = dict(attention_mask=m)
    with pytest.raises(NotImplementedError):
        te(ids, **kw)
    assert te.calls == []


@pytest.mark.parametrize("bad", [-1, T.TINY.vocab_size, 10 ** 6])
def test_out_of_range_ids_raise_before_native(bad):
    te = _fake_encoder()
    ids = T.padded_ids((6, 6), 6, T.TINY.vocab_size, T.TINY_PAD, 2)
    ids[1, 2] = bad
    with pytest.raises(ValueError):
        te(ids)
    with pytest.raises(ValueError):
        te.embed_tokens(ids)
    assert te.calls == []


# ------------------------------------------------------------------ seam
class _RefEncoder(torch.nn.Module):
    """Stands in for the reference Qwen3Model: an embedding and one linear."""

    def __init__(self):
        super().__init__()
        self.embed_tokens = torch.nn.Embedding(T.TINY.vocab_size, T.TINY.hidden_size)
        self.proj = torch.nn.Linear(T.TINY.hidden_size, T.TINY.hidden_size)

    def forward(self, input_ids=None, lyric_attention_mask=None, **kw):
        return types.SimpleNamespace(last_hidden_state=self.proj(self.embed_tokens(input_ids)))


def test_swap_wrapper_fallback_state_dict_and_embed_routing(caplog):
    from ace355.modswap import NativeTextEncoderSwap
    ref = _RefEncoder()
    fake = _fake_encoder()
    sw = NativeTextEncoderSwap(fake, ref, "text_encoder")
    assert list(sw.state_dict().keys()) == list(ref.state_dict().keys())
    ids = T.padded_ids((5, 5), 5, T.TINY.vocab_size, T.TINY_PAD, 4)
    out = sw(input_ids=ids, lyric_attention_mask=None).last_hidden_state
    assert out.dtype == torch.bfloat16 and sw.native_calls == 1
    e = sw.embed_tokens(ids)
    assert torch.equal(e, fake.embed_tokens(ids)) and fake.calls[-1][0] == "embed" and sw.native_calls == 2
    assert sw.embed_tokens.weight is ref.embed_tokens.weight
    # an unsupported call falls back to the PyTorch module, for the forward and for embed_tokens
    with caplog.at_level(logging.WARNING, logger="ace355"):
        fb = sw(input_ids=ids, output_hidden_states=True).last_hidden_state
        assert torch.equal(fb, ref(input_ids=ids).last_hidden_state)
        fake.embed_tokens = lambda _ids: (_ for _ in ()).throw(RuntimeError("boom"))
        fe = sw.embed_tokens(ids)
    assert torch.equal(fe, ref.embed_tokens(ids)) and sw.native_failures == 2
    # reloading the parent's weights keeps the reference's key names
    sw.load_state_dict(ref.state_dict())


def test_init_native_text_encoder_refuses_cpu_offload_and_cpu_device():
    from ace355.backend import NativeTextEncoderMixin

    class Host(NativeTextEncoderMixin):
        pass

    for offload, dev in ((True, "cuda:0"), (False, "cpu")):
        h = Host()
        h.text_encoder, h.device, h.offload_to_cpu = _RefEncoder(), dev, offload
        before = h.text_encoder
        assert h._init_native_text_encoder() is False
        assert h.text_encoder is before and h.use_native_text_encoder is False


def test_init_native_text_encoder_never_raises(monkeypatch):
    from ace355 import modswap
    from ace355.backend import NativeTextEncoderMixin

    class Host(NativeTextEncoderMixin):
        pass

    h = Host()
    h.text_encoder, h.device, h.offload_to_cpu = _RefEncoder(), "cuda:0", False
    before = h.text_encoder

    def boom(*a, **k):
        raise RuntimeError("no library")
    monkeypatch.setattr(modswap, "swap_in_text_encoder", boom)
    assert h._init_native_text_encoder() is False and h.text_encoder is before
