"""GPU: the native text encoder (transformers' Qwen3Model, the reference's Qwen3-Embedding-0.6B) against fixture G19 and the oracle.

Every parity gate is the project's rule (tests/_drift.py): below 2 x the oracle's own bf16-storage drift, per sequence and over the whole
tensor, pad rows included (the reference passes no mask, and the DiT attends the pad rows' outputs).  The tiny drift is measured in the same
run; the full-size drift is G19's (an fp32 CPU run of the 0.6B stack is minutes).
"""
import numpy as np
import pytest
import torch

import _drift
import _textenc_oracle as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g19():
    return T.load_g19()


@pytest.fixture(scope="module")
def tiny(gpu_device):
    from ace355 import weightgen
    from ace355.textenc import NativeTextEncoder
    w = T.weights(T.TINY, T.TINY_SEED)
    te = NativeTextEncoder(T.TINY, gpu_device)
    te.load_state_dict(w)
    yield te, w, weightgen.checksum(w)
    te.close()


@pytest.fixture(scope="module")
def full(gpu_device):
    """The published 0.6B shape with G19's weights, streamed tensor by tensor (2.4 GB of fp32 on the host at no point at once)."""
    from ace355 import native, weightgen
    from ace355.textenc import NativeTextEncoder
    te = NativeTextEncoder(T.FULL, gpu_device)
    wsum, table = 0.0, None
    for name, shape in T.FULL.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, T.FULL.hidden_size, seed=T.FULL_SEED, mode="test")[name].contiguous()
        wsum += float(wt.double().abs().sum())
        if name == "embed_tokens.weight":
            table = wt.to(torch.bfloat16)
        native.check(te._lib.ace355_textenc_load_tensor(te._h, name.encode(), native.ptr(wt), native.DTYPE_F32, wt.numel(), 0), name)
    native.check(te._lib.ace355_textenc_finalize(te._h), "finalize")
    yield te, wsum, table
    te.close()


def _gate(what, out, ref, drift_seq, drift_all):
    """Per sequence and whole tensor: relative L2 < 2 x drift (prints measured / drift)."""
    for b in range(ref.shape[0]):
        _drift.check(f"{what} sequence {b}", T.rel(out[b], ref[b]), float(drift_seq[b]))
    _drift.check(f"{what} whole tensor", T.rel(out, ref), float(drift_all))


@pytest.mark.parametrize("case", ["tiny_a", "tiny_b"])
def test_tiny_parity_vs_g19(tiny, g19, case):
    te, w, wsum = tiny
    assert abs(wsum - float(g19["tiny_checksum"])) <= 1e-9 * wsum
    ids = torch.from_numpy(g19[f"{case}_ids"]).long()
    ref = torch.from_numpy(g19[f"{case}_out"])
    out = te(ids).last_hidden_state
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape and out.device.type == "cuda"
    emu = _drift.emulated(T.text_encoder, T.TINY, w, ids)
    drift = [T.rel(emu[b], ref[b]) for b in range(ids.shape[0])]
    _gate(case, out.float().cpu(), ref, drift, T.rel(emu, ref))


def test_full_parity_vs_g19(full, g19):
    te, wsum, _table = full
    assert abs(wsum - float(g19["full_checksum"])) <= 1e-9 * wsum
    ids = torch.from_numpy(g19["full_ids"]).long()
    ref = torch.from_numpy(g19["full_out"])
    out = te(input_ids=ids.cuda(), lyric_attention_mask=None).last_hidden_state
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape
    _gate("full (0.6B shape, lengths 256 / 131 / 7)", out.float().cpu(), ref, g19["full_drift"], float(g19["full_drift_all"]))


def test_embed_tokens_bit_exact(full):
    te, _wsum, table = full
    V = T.FULL.vocab_size
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, V, (8, 2048), generator=g)
    ids[0, 0], ids[3, 100], ids[7, 2047] = 0, V - 1, V - 1
    out = te.embed_tokens(ids.cuda())
    assert out.dtype == torch.bfloat16 and out.shape == (8, 2048, T.FULL.hidden_size)
    exp = table[ids]
    assert torch.equal(out.cpu().view(torch.int16), exp.view(torch.int16))


def test_causality_and_batch_independence(tiny):
    te = tiny[0]
    V, S, p = T.TINY.vocab_size, 150, 70
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (3, S), generator=g)
    a = te(ids).last_hidden_state.cpu()
    b = te(ids).last_hidden_state.cpu()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the same call twice must give the same bits"
    ids2 = ids.clone()
    ids2[0, p + 1:] = torch.randint(0, V, (S - p - 1,), generator=g)
    c = te(ids2).last_hidden_state.cpu()
    assert torch.equal(c[0, :p + 1].view(torch.int16), a[0, :p + 1].view(torch.int16)), "rows <= p must not see later tokens"
    assert all(not torch.equal(c[0, r], a[0, r]) for r in range(p + 1, S)), "rows after p must change"
    assert torch.equal(c[1:].view(torch.int16), a[1:].view(torch.int16)), "other sequences must not see sequence 0"
    ids3 = ids.clone()
    ids3[1] = torch.randint(0, V, (S,), generator=g)
    d = te(ids3).last_hidden_state.cpu()
    assert torch.equal(d[0].view(torch.int16), a[0].view(torch.int16)) and torch.equal(d[2].view(torch.int16), a[2].view(torch.int16))
    assert not torch.equal(d[1], a[1])


@pytest.mark.parametrize("S", [1, 64, 65, 256])
def test_sequence_length_edges(tiny, S):
    te, w, _ = tiny
    lengths = (S, max(1, S // 3))
    ids = T.padded_ids(lengths, S, T.TINY.vocab_size, T.TINY_PAD, 100 + S)
    ref = T.text_encoder(T.TINY, w, ids)
    emu = _drift.emulated(T.text_encoder, T.TINY, w, ids)
    out = te(ids).last_hidden_state.float().cpu()
    _gate(f"S = {S}", out, ref, [T.rel(emu[b], ref[b]) for b in range(len(lengths))], T.rel(emu, ref))


def test_bad_ids_refused_then_next_call_matches(tiny):
    import ctypes as C
    from ace355 import native
    te = tiny[0]
    ids = T.padded_ids((40, 12), 40, T.TINY.vocab_size, T.TINY_PAD, 5)
    good = te(ids).last_hidden_state.cpu()
    for bad_id in (T.TINY.vocab_size, -1):
        bad = ids.clone()
        bad[1, 3] = bad_id
        with pytest.raises(ValueError):
            te(bad)
        with pytest.raises(ValueError):
            te.embed_tokens(bad)
        # the library refuses them too, before any launch
        b32 = bad.to(torch.int32).contiguous()
        out = torch.empty(2, 40, T.TINY.hidden_size, device="cuda", dtype=torch.bfloat16)
        rc = te._lib.ace355_textenc_encode(te._h, C.cast(b32.data_ptr(), C.POINTER(C.c_int32)), 2, 40, native.ptr(out),
                                           native.current_stream_ptr())
        assert rc == 1 and "outside" in native.last_error()
    again = te(ids).last_hidden_state.cpu()
    assert torch.equal(again.view(torch.int16), good.view(torch.int16))


def test_unsupported_head_layout_refused(gpu_device):
    from ace355.config import TextEncoderConfig
    from ace355.textenc import NativeTextEncoder
    for kw in (dict(num_attention_heads=4, num_key_value_heads=4), dict(head_dim=64)):
        with pytest.raises(NotImplementedError):
            NativeTextEncoder(TextEncoderConfig(**{**T.TINY.__dict__, **kw}), gpu_device)


def test_chain_text_encoder_to_condition_encoder(tiny, gpu_device):
    """Caption states and lyric embeddings from the native text encoder feed the native condition encoder; the oracle chain runs the
    same steps in fp32 (and in its bf16-storage mode for the drift)."""
    import ace355
    from ace355 import weightgen
    from ace355.cond import NativeCondEncoder
    from oracle import cond as o_cond
    te, tw, _ = tiny
    ckw = dict(hidden_size=256, intermediate_size=768, num_attention_heads=2, num_key_value_heads=1, head_dim=128, text_hidden_dim=256,
               timbre_hidden_dim=64, num_lyric_encoder_hidden_layers=2, num_timbre_encoder_hidden_layers=2, sliding_window=16)
    ccfg = ace355.CondConfig(**ckw)
    cw = weightgen.make_dit_weights(ccfg.weight_shapes(), ccfg.hidden_size, seed=41, mode="test")
    B, Lt, Ll = 2, 24, 40
    text_ids = T.padded_ids((24, 9), Lt, T.TINY.vocab_size, T.TINY_PAD, 42)
    lyric_ids = T.padded_ids((40, 17), Ll, T.TINY.vocab_size, 0, 43)
    tmask = (torch.arange(Lt)[None] < torch.tensor([24, 9])[:, None]).long()
    lmask = (torch.arange(Ll)[None] < torch.tensor([40, 17])[:, None]).long()
    g = torch.Generator().manual_seed(44)
    refer = torch.randn(2, 30, 64, generator=g)
    order = torch.tensor([0, 1])

    enc = NativeCondEncoder(ccfg, gpu_device)
    enc.load_state_dict(cw)
    n_text = te(text_ids).last_hidden_state
    n_lyr = te.embed_tokens(lyric_ids)
    n_h, _n_m = enc(n_text, tmask, n_lyr, lmask, refer, order)

    ocfg = o_cond.CondConfig(**ckw)

    def chain(_cfg, w, tw_, cw_):
        text = T.text_encoder(T.TINY, tw_, text_ids)
        lyr = tw_["embed_tokens.weight"][lyric_ids]
        return o_cond.condition_encoder(ocfg, cw_, text, tmask, lyr, lmask, refer, order)[0]

    ref = chain(None, None, tw, cw)
    from oracle import dit as o_dit
    with o_dit.bf16_storage():
        emu = chain(None, None, o_dit.bf16_weights(tw), o_dit.bf16_weights(cw))
    _drift.check("text encoder -> condition encoder", T.rel(n_h.float().cpu(), ref), T.rel(emu, ref))


def test_handler_seam_matches_direct_calls(tiny, gpu_device):
    import ace355
    from ace355 import weightgen
    from ace355.backend import NativeHandler
    from ace355.textenc import NativeTextEncoder
    _te, tw, _ = tiny
    kw = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)
    dcfg = ace355.DitConfig(**kw)
    dw = weightgen.make_dit_weights(dcfg.weight_shapes(), dcfg.hidden_size, seed=1, mode="test")
    null = weightgen.make_null_condition_emb(dcfg.hidden_size, seed=1)
    h = NativeHandler()
    msg, ok = h.initialize_service(dcfg, dw, null, device="cuda", text_encoder_config=T.TINY, text_encoder_state_dict=tw)
    assert ok, msg
    direct = NativeTextEncoder(T.TINY, gpu_device)
    direct.load_state_dict(tw)
    ids = T.padded_ids((33, 5, 20), 33, T.TINY.vocab_size, T.TINY_PAD, 9)
    lyr = torch.randint(0, T.TINY.vocab_size, (2, 300), generator=torch.Generator().manual_seed(10))
    a = h.infer_text_embeddings(ids.cuda())
    b = direct(input_ids=ids.cuda(), lyric_attention_mask=None).last_hidden_state
    assert a.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
    c = h.infer_lyric_embeddings(lyr.cuda())
    d = direct.embed_tokens(lyr.cuda())
    assert torch.equal(c.view(torch.int16), d.view(torch.int16))
    direct.close()
