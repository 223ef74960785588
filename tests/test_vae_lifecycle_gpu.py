"""GPU: the load / finalize / run lifecycle of the VAE handle (csrc/vae.hip), driven through the raw C calls on the small configuration:
the refusals with their texts, bit-equal output whatever the order and the residence of the loaded tensors, a full reload, and the
re-finalize rule - finalize consumes the loaded tensors, so anything less than a full reload is refused by host bookkeeping."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
T, FRAMES = 5, 3   # latent frames decoded; frames of audio encoded
ERR_INVALID, ERR_STATE = 1, 3


def _cfg():
    import ace355
    return ace355.VaeConfig(**SMALL)


def _weights(seed, encoder=True):
    from ace355 import weightgen
    cfg = _cfg()
    return weightgen.make_vae_weights({**cfg.weight_shapes(), **(cfg.encoder_weight_shapes() if encoder else {})}, seed=seed, mode="test")


def _new(device):
    from ace355.vae import NativeVae
    return NativeVae(_cfg(), device)


def _load(vae, name, t, numel=None):
    """Raw ``ace355_vae_load_tensor`` of an fp32 tensor, host or device; returns (rc, last error)."""
    from ace355 import native
    t = t.contiguous()
    with torch.cuda.device(vae.device):
        rc = vae._lib.ace355_vae_load_tensor(vae._h, name.encode(), native.ptr(t), native.DTYPE_F32, t.numel() if numel is None else numel,
                                             1 if t.is_cuda else 0)
    return rc, native.last_error()


def _load_all(vae, w):
    for n, t in w.items():
        rc, err = _load(vae, n, t)
        assert rc == 0, (n, err)


def _finalize(vae):
    from ace355 import native
    with torch.cuda.device(vae.device):
        return vae._lib.ace355_vae_finalize(vae._h), native.last_error()


def _decode(vae, z):
    """Raw ``ace355_vae_decode``; returns (rc, last error, waveform)."""
    from ace355 import native
    zd = z.to(vae.device, torch.float32).contiguous()
    out = torch.zeros(z.shape[0], 2, vae.hop * z.shape[2], device=vae.device)
    with torch.cuda.device(vae.device):
        rc = vae._lib.ace355_vae_decode(vae._h, native.ptr(zd), z.shape[0], z.shape[2], native.ptr(out), native.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, native.last_error(), out.cpu()


@pytest.fixture(scope="module")
def ref(gpu_device):
    """Inputs, and what handles loaded through NativeVae.load_state_dict give for them: seed A both halves, seed B the decode."""
    cfg = _cfg()
    z = torch.randn(1, 64, T, generator=torch.Generator().manual_seed(7))
    audio = 0.3 * torch.randn(1, 2, cfg.hop * FRAMES, generator=torch.Generator().manual_seed(8))
    out = {"z": z, "audio": audio, "A": _weights(21), "B": _weights(22)}
    for k in ("A", "B"):
        vae = _new(gpu_device)
        try:
            vae.load_state_dict(out[k])
            out["wav" + k] = vae.decode(z).cpu()
            out["mean" + k] = vae.encode(audio, sample=False).cpu()
        finally:
            vae.close()
    assert not torch.equal(out["wavA"], out["wavB"]) and bool(torch.isfinite(out["wavA"]).all()) and bool(torch.isfinite(out["meanA"]).all())
    return out


def test_refusals_keep_their_texts(ref, gpu_device):
    w = {k: t for k, t in ref["A"].items() if k.startswith("decoder.")}
    missing = "decoder.block.1.res_unit2.conv1.weight_g"
    assert missing in w
    vae = _new(gpu_device)
    try:
        rc, err, _ = _decode(vae, ref["z"])
        assert rc == ERR_STATE and err == "vae_decode: call ace355_vae_finalize first", (rc, err)
        rc, err = _load(vae, "quantizer.conv1.bias", w[missing])
        assert rc == ERR_INVALID and err == "vae_load_tensor: unknown tensor name 'quantizer.conv1.bias' (decoder.* / encoder.* expected)", (rc, err)
        _load_all(vae, {k: t for k, t in w.items() if k != missing})
        rc, err = _finalize(vae)
        assert rc == ERR_STATE and err == f"vae_finalize: missing tensor '{missing}'", (rc, err)
        rc, err, _ = _decode(vae, ref["z"])
        assert rc == ERR_STATE and err == "vae_decode: call ace355_vae_finalize first", (rc, err)
        n = w[missing].numel()
        rc, err = _load(vae, missing, w[missing], numel=n - 1)
        assert rc == 0, err
        rc, err = _finalize(vae)
        assert rc == ERR_INVALID and err == f"vae_finalize: wrong size for '{missing}': got {n - 1}, expected {n}", (rc, err)
        # a refused finalize consumed nothing: the one tensor put right, the handle seals and decodes
        rc, err = _load(vae, missing, w[missing])
        assert rc == 0, err
        rc, err = _finalize(vae)
        assert rc == 0, err
        rc, err, wav = _decode(vae, ref["z"])
        assert rc == 0 and torch.equal(wav, ref["wavA"]), err
        # no encoder.* tensor was loaded: as test_vae_gpu.py::test_encode_requires_encoder_weights
        with pytest.raises(RuntimeError, match="encoder"):
            vae.encode(torch.zeros(1, 2, vae.hop * 4))
    finally:
        vae.close()


@pytest.mark.parametrize("how", ["reversed", "device"])
def test_order_and_residence_do_not_change_the_bits(ref, gpu_device, how):
    w = ref["A"]
    if how == "reversed":
        w = dict(reversed(list(w.items())))
    else:
        w = {k: t.to(gpu_device) for k, t in w.items()}
    vae = _new(gpu_device)
    try:
        _load_all(vae, w)
        rc, err = _finalize(vae)
        assert rc == 0, err
        assert torch.equal(vae.decode(ref["z"]).cpu(), ref["wavA"])
        assert torch.equal(vae.encode(ref["audio"], sample=False).cpu(), ref["meanA"])
    finally:
        vae.close()


def test_full_reload_replaces_the_weights(ref, gpu_device):
    vae = _new(gpu_device)
    try:
        for k in ("A", "B"):
            _load_all(vae, ref[k])
            rc, err = _finalize(vae)
            assert rc == 0, (k, err)
            rc, err, wav = _decode(vae, ref["z"])
            assert rc == 0 and torch.equal(wav, ref["wav" + k]), (k, err)
        assert torch.equal(vae.encode(ref["audio"], sample=False).cpu(), ref["meanB"])
    finally:
        vae.close()


def test_partial_reload_is_refused(ref, gpu_device):
    """Finalize erased the tensors it consumed, so one tensor loaded again leaves the next finalize without the rest: ERR_STATE from the
    host's bookkeeping (ace355_vae_finalize checks every name and size before its first device call), the handle stays unfinalized, and a
    full reload seals it again."""
    vae = _new(gpu_device)
    try:
        _load_all(vae, ref["A"])
        rc, err = _finalize(vae)
        assert rc == 0, err
        name = "decoder.block.0.conv_t1.weight_v"
        rc, err = _load(vae, name, ref["B"][name])
        assert rc == 0, err
        rc, err = _finalize(vae)
        assert rc == ERR_STATE and err.startswith("vae_finalize: missing tensor '"), (rc, err)
        rc, err, _ = _decode(vae, ref["z"])
        assert rc == ERR_STATE and err == "vae_decode: call ace355_vae_finalize first", (rc, err)
        with pytest.raises(RuntimeError):
            vae.encode(ref["audio"], sample=False)
        _load_all(vae, ref["B"])
        rc, err = _finalize(vae)
        assert rc == 0, err
        rc, err, wav = _decode(vae, ref["z"])
        assert rc == 0 and torch.equal(wav, ref["wavB"]), err
    finally:
        vae.close()
