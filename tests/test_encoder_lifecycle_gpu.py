"""GPU: the load / finalize / run lifecycle that the four encoder-stack handles (cond, detok, tok, textenc) share through
csrc/encoder.hip, driven through the raw C calls on tiny handles: name and size checks, the canonical layer index, the loaded count,
the finalize gate, and bit-equal output against a handle loaded through the Python owner class."""
import ctypes as C

import pytest
import torch

import _textenc_oracle as T

pytestmark = pytest.mark.gpu

TINY = dict(hidden_size=256, intermediate_size=768, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
# the four spellings of a layer index that are not the canonical decimal form of a layer below n_layers = 2
BAD_INDICES = ("01", "1x", "", "2")


class Kind:
    """One handle kind: how to make the owner object, its weights, the layer-key prefix and one seeded call."""

    def __init__(self, what, make, weights, prefix, run, ignored=()):
        self.what, self.make, self.weights, self.prefix, self.run, self.ignored = what, make, weights, prefix, run, ignored


def _kinds():
    import ace355
    from ace355 import weightgen
    from ace355.config import TextEncoderConfig
    from ace355.cond import NativeCondEncoder
    from ace355.lmhints import NativeAudioTokenizer, NativeDetokenizer
    from ace355.textenc import NativeTextEncoder
    from oracle import detok as o_detok

    def gen(shapes, seed):
        return weightgen.make_dit_weights(shapes, 256, seed=seed, mode="test")

    ccfg = ace355.CondConfig(**TINY, text_hidden_dim=64, timbre_hidden_dim=64, num_lyric_encoder_hidden_layers=2,
                             num_timbre_encoder_hidden_layers=2, sliding_window=16)
    dcfg = ace355.DetokConfig(**TINY)
    tcfg = TextEncoderConfig(**TINY, num_hidden_layers=2, vocab_size=T.TINY.vocab_size)
    g = torch.Generator().manual_seed(3)
    text, lyric, refer = torch.randn(2, 9, 64, generator=g), torch.randn(2, 70, 64, generator=g), torch.randn(3, 33, 64, generator=g)
    tmask = (torch.arange(9)[None] < torch.tensor([9, 4])[:, None]).long()
    lmask = (torch.arange(70)[None] < torch.tensor([70, 21])[:, None]).long()
    order = torch.tensor([0, 1, 1])
    x_det, x_tok = torch.randn(2, 7, 256, generator=g), torch.randn(2, 7 * dcfg.pool_window_size, 64, generator=g)
    ids = T.padded_ids((65, 20), 65, tcfg.vocab_size, tcfg.vocab_size - 1, 4)
    return {
        "cond": Kind("cond", lambda dev: NativeCondEncoder(ccfg, dev), gen(ccfg.weight_shapes(), 31), "lyric_encoder.",
                     lambda o: o(text, tmask, lyric, lmask, refer, order)[0],
                     ignored=("lyric_encoder.special_token", "timbre_encoder.special_token")),
        "detok": Kind("detok", lambda dev: NativeDetokenizer(dcfg, dev), gen(dcfg.weight_shapes(), 32), "", lambda o: o(x_det)),
        "tok": Kind("tok", lambda dev: NativeAudioTokenizer(dcfg, dev),
                    gen(o_detok.tok_weight_shapes(o_detok.DetokConfig(**TINY)), 33), "attention_pooler.", lambda o: o.pool(x_tok)),
        "textenc": Kind("textenc", lambda dev: NativeTextEncoder(tcfg, dev), gen(tcfg.weight_shapes(), 34), "",
                        lambda o: o(ids).last_hidden_state),
    }


@pytest.fixture(scope="module")
def kinds(gpu_device):
    return _kinds()


def _load(obj, what, name, t, numel=None):
    """Raw ``<what>_load_tensor`` of an fp32 host tensor; returns (rc, last error)."""
    from ace355 import native
    t = t.contiguous()
    rc = getattr(obj._lib, f"ace355_{what}_load_tensor")(obj._h, name.encode(), native.ptr(t), native.DTYPE_F32,
                                                        t.numel() if numel is None else numel, 0)
    return rc, native.last_error()


def _finalize(obj, what):
    from ace355 import native
    return getattr(obj._lib, f"ace355_{what}_finalize")(obj._h), native.last_error()


@pytest.mark.parametrize("what", ["cond", "detok", "tok", "textenc"])
def test_lifecycle(kinds, gpu_device, what):
    k = kinds[what]
    w = {n: t for n, t in k.weights.items() if n not in k.ignored}
    N = len(w)
    missing = k.prefix + "layers.1.mlp.up_proj.weight"
    assert missing in w
    obj = k.make(gpu_device)
    try:
        rc, err = _load(obj, what, k.prefix + "no_such.weight", w[missing])
        assert rc != 0 and "unknown tensor name" in err, err
        rc, err = _load(obj, what, missing, w[missing], numel=w[missing].numel() - 1)
        assert rc != 0 and "wrong element count" in err, err
        for n, t in w.items():
            if n != missing:
                rc, err = _load(obj, what, n, t)
                assert rc == 0, (n, err)
        # no other spelling of the missing tensor's layer index is a layer, and none of them counts as a loaded tensor
        for bad in BAD_INDICES:
            rc, err = _load(obj, what, missing.replace("layers.1.", f"layers.{bad}."), w[missing])
            assert rc != 0 and "unknown tensor name" in err, (bad, err)
        for n in k.ignored:   # parameters the reference module never reads: accepted, not counted
            rc, err = _load(obj, what, n, torch.zeros(1, 1, 256))
            assert rc == 0, (n, err)
        rc, err = _finalize(obj, what)
        assert rc != 0 and f"{N - 1} of {N} tensors loaded" in err, err
        with pytest.raises(RuntimeError, match="finalize first"):
            k.run(obj)
        rc, err = _load(obj, what, missing, w[missing])
        assert rc == 0, err
        rc, err = _finalize(obj, what)
        assert rc == 0, err
        out = k.run(obj)
        # a tensor loaded again un-finalizes the handle
        rc, err = _load(obj, what, missing, w[missing])
        assert rc == 0, err
        with pytest.raises(RuntimeError, match="finalize first"):
            k.run(obj)
        rc, err = _finalize(obj, what)
        assert rc == 0, err
        assert torch.equal(k.run(obj), out)
        fresh = k.make(gpu_device)
        try:
            fresh.load_state_dict(k.weights)
            ref = k.run(fresh)
        finally:
            fresh.close()
        assert out.shape == ref.shape and bool(torch.isfinite(out.float()).all()) and torch.equal(out, ref)
    finally:
        obj.close()


def test_textenc_more_layers_than_mask_bits(gpu_device):
    """A causal stack may have more than 64 layers (the sliding-layer mask of the bidirectional stacks has 64 bits and is not read on the
    causal path): 65 tiny layers create, load and encode."""
    from ace355 import native, weightgen
    from ace355.config import TextEncoderConfig
    from ace355.textenc import NativeTextEncoder
    cfg = TextEncoderConfig(**TINY, num_hidden_layers=65, vocab_size=T.TINY.vocab_size)
    one = TextEncoderConfig(**TINY, num_hidden_layers=1, vocab_size=T.TINY.vocab_size)
    w1 = weightgen.make_dit_weights(one.weight_shapes(), 256, seed=35, mode="test")
    te = NativeTextEncoder(cfg, gpu_device)
    try:
        for name in cfg.weight_shapes():   # every layer carries layer 0's tensors
            parts = name.split(".")
            src = name if parts[0] != "layers" else ".".join(["layers", "0"] + parts[2:])
            rc, err = _load(te, "textenc", name, w1[src])
            assert rc == 0, (name, err)
        rc, err = _finalize(te, "textenc")
        assert rc == 0, err
        ids = T.padded_ids((8,), 8, cfg.vocab_size, cfg.vocab_size - 1, 6).to(torch.int32).contiguous()
        out = torch.empty(1, 8, 256, device=gpu_device, dtype=torch.bfloat16)
        rc = te._lib.ace355_textenc_encode(te._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int32)), 1, 8, native.ptr(out),
                                           native.current_stream_ptr())
        assert rc == 0, native.last_error()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
    finally:
        te.close()
