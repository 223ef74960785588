"""CPU: the audio input stage's plan, ABI structs, WAV parser, tap table, reference cut and handler seam (ace355.audio_in,
csrc/audio_in_plan.h, backend.NativeAudioInMixin).  The kernel itself: tests/test_audio_in_gpu.py."""
import ctypes
import logging
import math
import os
import random
import subprocess

import pytest
import torch

import _audio_in_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (44100, 32000, 16000, 96000, 88200, 48000)
LENGTHS = (1, 5, 2940, 3001)   # 2940 = 20 x 147: whole blocks at 44.1 kHz
EXPECTED_K = {44100: 13, 32000: 13, 16000: 13, 96000: 25, 88200: 23}


@pytest.fixture(scope="module")
def tables():
    import ace355  # noqa: F401
    from ace355 import audio_in
    return {sr: audio_in.tap_table(sr) for sr in RATES + (11025, 352800)}


def _plan(tab, frames, fmt="s16", channels=2):
    from ace355 import native
    return native.audio_in_plan(fmt, channels, frames, tab["o"], tab["n"], tab["K"], tab["width"])


# ---------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("sr", RATES)
def test_plan_output_length(tables, sr):
    from ace355 import audio_in
    tab = tables[sr]
    o, n = O.ratio(sr)
    assert (tab["o"], tab["n"]) == (o, n)
    for L in LENGTHS:
        p = _plan(tab, L)
        assert p["out_frames"] == math.ceil(n * L / o) == audio_in.output_frames(L, sr), (sr, L)
        assert p["passthrough"] == int(sr == 48000) and p["threads"] == 256


@pytest.mark.parametrize("sr,L", [(44100, 3001), (44100, 44100), (96000, 3001), (16000, 5), (11025, 3001), (352800, 30011), (48000, 3001)])
def test_plan_grid_covers_every_output_once_and_every_tap_is_staged(tables, sr, L):
    """Tile t owns [t tile, min(out, (t + 1) tile)): together [0, out) without overlap, and every input frame an output of the tile reads
    through the compacted table lies inside the span the tile stages."""
    tab = tables[sr]
    p = _plan(tab, L)
    tile, out, o, n = p["tile"], p["out_frames"], tab["o"], tab["n"]
    assert p["grid"] == -(-out // tile) and (p["grid"] - 1) * tile < out <= p["grid"] * tile
    seen = torch.zeros(out, dtype=torch.int32)
    for t in range(p["grid"]):
        lo, hi = t * tile, min(out, (t + 1) * tile)
        seen[lo:hi] += 1
        if p["passthrough"]:
            continue
        j = torch.arange(lo, hi)
        b, ph = j // n, j % n
        start = (b - lo // n) * o + tab["first"][ph].long()   # LDS slot of the first tap: slot 0 holds input frame (lo // n) o - width
        assert int(start.min()) >= 0 and int(start.max()) + tab["K"] <= p["span"], (sr, t)
    assert bool((seen == 1).all())
    assert p["lds_bytes"] == 8 * p["span"] + (4 * n * ((tab["K"] | 1) + 1) if p["table_in_lds"] else 0) <= 60 * 1024


def test_plan_table_in_lds_or_global_and_tile_choice(tables):
    assert _plan(tables[44100], 3001)["table_in_lds"] == 1                     # 160 phases x 13 taps: 9 KB
    assert _plan(tables[11025], 3001)["table_in_lds"] == 0                     # 640 phases x 13 taps: 36 KB > 24 KB, read from global memory
    assert _plan(tables[48000], 3001)["table_in_lds"] == 0 and _plan(tables[48000], 3001)["lds_bytes"] == 0
    assert _plan(tables[44100], 3001)["tile"] == 1024
    p = _plan(tables[352800], 3001)                                           # o = 147, n = 20: 1024 outputs would read 7 900 input frames
    assert p["tile"] == 512 and 8 * p["span"] <= 60 * 1024 < 8 * ((1024 + 18) // 20 * 147 + 2 * tables[352800]["width"] + 147)
    assert _plan(tables[44100], 3001) == _plan(tables[44100], 3001)
    assert _plan(tables[44100], 3001, "f32", 6)["tile"] == _plan(tables[44100], 3001, "u8", 1)["tile"]   # neither format nor channels move it


REFUSALS = [
    ("a rate of zero", dict(o=0, n=1, K=1, width=1), "sample rate"),
    ("a negative rate", dict(o=-147, n=160, K=13, width=7), "sample rate"),
    ("no output phases", dict(o=147, n=0, K=13, width=7), "sample rate"),
    ("not in lowest terms", dict(o=294, n=320, K=13, width=7), "lowest terms"),
    ("n does not divide 48000", dict(o=1, n=7, K=13, width=7), "lowest terms"),
    ("a coprime rate (47999 Hz)", dict(o=47999, n=48000, K=13, width=7), "2^22"),
    ("22255 Hz", dict(o=4451, n=9600, K=13, width=7), "2^22"),
    ("no frames", dict(frames=0), "frames"),
    ("negative frames", dict(frames=-5), "frames"),
    ("frames past 2^36", dict(frames=(1 << 36) + 1), "frames"),
    ("more tiles than a grid holds", dict(o=1, n=48000, K=13, width=7, frames=1 << 36), "tiles"),
    ("a table at 48 kHz", dict(o=1, n=1, K=13, width=7), "K / width"),
    ("no table off 48 kHz", dict(K=0, width=0), "K / width"),
    ("more taps than the dense table", dict(K=162), "K / width"),
    ("a span beyond LDS", dict(o=1000, n=1, K=12121, width=6061), "LDS"),
    ("an unknown format", dict(format=5), "format"),
    ("no channels", dict(channels=0), "channels"),
]


@pytest.mark.parametrize("what,fields,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refusals(what, fields, text):
    from ace355 import native
    rq = native.AudioInRequestC(format=1, channels=2, o=147, n=160, K=13, width=7, frames=3001)
    out = native.AudioInPlanInfoC()
    assert native.lib().ace355_audio_in_plan(ctypes.byref(rq), ctypes.byref(out)) == 0
    for k, v in fields.items():
        setattr(rq, k, v)
    assert native.lib().ace355_audio_in_plan(ctypes.byref(rq), ctypes.byref(out)) == 1, what
    assert "audio_in_plan" in native.last_error() and text in native.last_error(), native.last_error()
    # the launch refuses what the plan refuses, before it touches a pointer
    assert native.lib().ace355_audio_in_run(ctypes.byref(rq), 4, 1 << 40, 0, 4, 4, 4, 4, None) == 1
    assert text in native.last_error()


def test_plan_null_arguments_and_the_cap_constant():
    from ace355 import audio_in, native
    assert native.lib().ace355_audio_in_plan(None, None) == 1
    assert native.AUDIO_IN_MAX_DENSE_TAPS == 1 << 22
    with pytest.raises(NotImplementedError, match="47999"):
        audio_in.tap_table(47999)          # refused on the host before an 18 GB table is built
    with pytest.raises(NotImplementedError):
        audio_in.rate_ratio(0)


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the two new structs, taken from the HEADER by the C compiler, vs the ctypes mirrors
    (the method of tests/test_abi.py::test_struct_layouts_match_header)."""
    from ace355 import native
    structs = {"ace355_audio_in_request": native.AudioInRequestC, "ace355_audio_in_plan_info": native.AudioInPlanInfoC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _t in ct._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("formats %d %d %d %d %d\\n", ACE355_PCM_U8, ACE355_PCM_S16, ACE355_PCM_S24, ACE355_PCM_S32, ACE355_PCM_F32);', "  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {r[0]: r[1:] for r in rows}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == ctypes.sizeof(ct), cname
        for fname, _t in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["formats"]] == list(range(5)) and native.PCM_FORMATS == ("u8", "s16", "s24", "s32", "f32")
    assert ctypes.sizeof(native.AudioInRequestC) == 32 and ctypes.sizeof(native.AudioInPlanInfoC) == 40


# ---------------------------------------------------------------------------------------------------- WAV parser
def _raw(fmt, channels, frames=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return O.float_to_pcm(torch.rand(frames * channels, generator=g) * 1.8 - 0.9, fmt)


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32"])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_wav_parser_every_format(fmt, channels):
    from ace355.audio_in import PcmInfo, parse_wav
    raw = _raw(fmt, channels)
    assert parse_wav(O.wav_bytes(raw, fmt, channels, 44100)) == PcmInfo(fmt, channels, 44100, 7, 44)
    assert parse_wav(O.wav_bytes(raw, fmt, channels, 96000, extensible=True)) == PcmInfo(fmt, channels, 96000, 7, 68)
    assert parse_wav(bytearray(O.wav_bytes(raw, fmt, channels, 8000))).offset == 44   # any bytes-like


def test_wav_parser_chunks_and_truncation():
    from ace355.audio_in import parse_wav
    raw = _raw("s16", 2)
    # an odd-sized unknown chunk ahead of data: its pad byte is skipped too
    w = O.wav_bytes(raw, "s16", 2, 32000, pre_chunks=[(b"LIST", b"abcde"), (b"fact", b"\x07\0\0\0")])
    info = parse_wav(w)
    assert info.offset == 44 + 8 + 6 + 8 + 4 and info.frames == 7 and w[info.offset:info.offset + len(raw)] == raw
    # an 18-byte fmt chunk (cbSize = 0), as float writers emit: the payload starts at byte 46, not a multiple of 4
    assert parse_wav(O.wav_bytes(_raw("f32", 1), "f32", 1, 48000, fmt_extra=b"\0\0")).offset == 46
    # a data chunk that claims more than the file holds is cut at the end of the file, whole frames only
    assert parse_wav(O.wav_bytes(raw, "s16", 2, 32000, data_size=0xFFFFFFFF)).frames == 7
    assert parse_wav(O.wav_bytes(raw[:-3], "s16", 2, 32000, data_size=4096)).frames == 6
    # a data chunk shorter than the file: what it says
    assert parse_wav(O.wav_bytes(raw, "s16", 2, 32000, data_size=8) + b"junk").frames == 2
    assert parse_wav(O.wav_bytes(b"", "s16", 2, 32000)).frames == 0


WAV_REFUSALS = {
    "ADPCM": lambda: O.wav_bytes(b"\0" * 64, "s16", 2, 44100, tag=2, bits=4),
    "float64": lambda: O.wav_bytes(b"\0" * 64, "f32", 2, 44100, bits=64),
    "zero channels": lambda: O.wav_bytes(b"\0" * 64, "s16", 0, 44100),
    "extensible ADPCM": lambda: O.wav_bytes(b"\0" * 64, "s16", 2, 44100, extensible=True, tag=2),
    "12-bit PCM": lambda: O.wav_bytes(b"\0" * 64, "s16", 2, 44100, bits=12),
    "RF64": lambda: b"RF64" + O.wav_bytes(b"\0" * 64, "s16", 2, 44100)[4:],
    "no data chunk": lambda: O.wav_bytes(b"\0" * 64, "s16", 2, 44100)[:36],
    "mp3": lambda: b"ID3\x04" + b"\0" * 64,
    "empty": lambda: b"",
}


@pytest.mark.parametrize("what", sorted(WAV_REFUSALS))
def test_wav_parser_refusals(what):
    from ace355.audio_in import find_payload
    with pytest.raises(NotImplementedError):
        find_payload(WAV_REFUSALS[what]())


def test_flac_payload_and_depth_refusal():
    """FLAC goes through the package's decoder; a stream deeper than 16 bits is refused before it is decoded."""
    import numpy as np
    from ace355.audio_in import PcmInfo, find_payload
    from ace355.audio_out import flac_encode_pcm16
    pcm = (np.arange(600, dtype=np.int16).reshape(300, 2) * 37) % 1000 - 500
    data = flac_encode_pcm16(pcm, 44100)
    payload, info = find_payload(data)
    assert info == PcmInfo("s16", 2, 44100, 300, 0) and payload.tobytes() == pcm.astype("<i2").tobytes()
    deep = bytearray(data)
    # STREAMINFO: bits per sample - 1 sits in the low bit of byte 20 and the high nibble of byte 21 (after 20 bits of rate, 3 of channels)
    deep[20] = (deep[20] & 0xFE) | ((23 >> 4) & 1)
    deep[21] = (deep[21] & 0x0F) | ((23 & 0xF) << 4)
    with pytest.raises(NotImplementedError, match="24 bits"):
        find_payload(bytes(deep))


# ---------------------------------------------------------------------------------------------------- tap table
@pytest.mark.parametrize("sr", [r for r in RATES if r != 48000])
def test_tap_table_is_the_dense_table_without_its_clamped_taps(tables, sr):
    tab = tables[sr]
    k64, raw, o, n, width = O.dense_table(sr)
    assert (tab["o"], tab["n"], tab["width"], tab["K"]) == (o, n, width, EXPECTED_K[sr])
    assert k64.shape == (n, 2 * width + o)
    k32 = k64.to(torch.float32)
    first, K = tab["first"].long(), tab["K"]
    assert tab["taps"].dtype == torch.float32 and tab["taps"].shape == (n, K) and tab["first"].dtype == torch.int32
    assert int(first.min()) >= 0 and int(first.max()) + K <= k64.shape[1]
    cols = first[:, None] + torch.arange(K)[None]
    assert torch.equal(tab["taps"], k32.gather(1, cols)), "kept taps differ from the oracle's dense fp32 table"
    kept = torch.zeros_like(k64, dtype=torch.bool).scatter_(1, cols, True)
    assert bool(kept[raw.abs() < 6].all()), "a tap with an unclamped window argument was dropped"
    assert float(k64[~kept].abs().max()) < 1e-20
    assert int((raw.abs() < 6).sum(dim=1).max()) == K                      # K is the widest phase, no wider
    assert abs(float(k64.sum(dim=1).mean()) - 1.0) < 2e-3                  # a phase passes DC at ~unit gain


def test_tap_table_at_48k_is_empty(tables):
    assert tables[48000] == {"o": 1, "n": 1, "K": 0, "width": 0, "first": None, "taps": None}


# ---------------------------------------------------------------------------------------------------- reference cut
@pytest.mark.parametrize("seconds", [4, 31, 95])
def test_reference_segments_against_the_reference_lines(seconds):
    from ace355.audio_in import reference_segments
    S = seconds * 48000 + 17
    wav = torch.stack([torch.arange(S, dtype=torch.float32), -torch.arange(S, dtype=torch.float32)])   # a sample names its own position
    random.seed(7)
    want = O.reference_cut(wav)
    after = random.random()
    random.seed(7)
    got = reference_segments(wav)
    assert random.random() == after, "not the reference's three draws"
    assert got.shape == (2, 30 * 48000) and torch.equal(got, want)
    if seconds == 4:
        assert math.ceil(30 * 48000 / S) == 8   # the clip is repeated 8 times first


# ---------------------------------------------------------------------------------------------------- seam
class _Parent:
    def process_src_audio(self, audio_file):
        return ("parent-src", audio_file)

    def process_reference_audio(self, audio_file):
        return ("parent-ref", audio_file)

    def process_target_audio(self, audio_file):
        return ("parent-target", audio_file)


def _host(loader, parent=True, on=True):
    from ace355.backend import NativeAudioInMixin
    cls = type("Host", (NativeAudioInMixin, _Parent) if parent else (NativeAudioInMixin,), {})
    h = cls()
    h.device = "cpu"
    h.use_native_audio_in = on
    h._native_load_audio = loader
    return h


def test_mixin_paths(caplog):
    from ace355.backend import NativeAudioInMixin, NativeHandler
    assert NativeAudioInMixin.use_native_audio_in is (os.environ.get("ACE355_AUDIO_IN", "") == "1")
    assert issubclass(NativeHandler, NativeAudioInMixin)
    loud = torch.full((2, 4 * 48000), 0.25)
    calls = []

    def loader(f):
        calls.append(f)
        return loud, 0.25
    h = _host(loader)
    for name in ("process_src_audio", "process_target_audio", "process_reference_audio"):
        assert getattr(h, name)(None) is None
    assert calls == []
    assert h.process_src_audio("a.wav") is loud and h.process_target_audio("b.wav") is loud
    random.seed(7)
    want = O.reference_cut(loud)
    random.seed(7)
    assert torch.equal(h.process_reference_audio("c.wav"), want)
    assert calls == ["a.wav", "b.wav", "c.wav"]
    # silent: the reference cut is None, the other two hand the tensor on (as the reference does)
    quiet = _host(lambda f: (torch.zeros(2, 480), 9e-7))
    assert quiet.process_reference_audio("q.wav") is None and quiet.process_src_audio("q.wav") is not None
    assert _host(lambda f: (loud, 1e-6)).process_reference_audio("q.wav") is not None   # (1e-6 itself is not below 1e-6)
    # errors of the reference's list: logged, None
    for exc in (OSError("gone"), RuntimeError("hip"), ValueError("empty")):
        def failing(f, exc=exc):
            raise exc
        with caplog.at_level(logging.WARNING, logger="ace355"):
            for name in ("process_src_audio", "process_target_audio", "process_reference_audio"):
                assert getattr(_host(failing), name)("x.wav") is None
    assert "gone" in caplog.text
    with pytest.raises(KeyError):   # anything else is a bug and propagates, as in the reference
        _host(lambda f: {}["x"]).process_src_audio("x.wav")


def test_mixin_not_implemented_reaches_the_parent_and_off_is_untouched(caplog):
    def unsupported(f):
        raise NotImplementedError("WAV: format tag 2")
    h = _host(unsupported)
    assert h.process_src_audio("x.wav") == ("parent-src", "x.wav")
    assert h.process_reference_audio("x.wav") == ("parent-ref", "x.wav")
    assert h.process_target_audio("x.wav") == ("parent-target", "x.wav")
    with caplog.at_level(logging.WARNING, logger="ace355"):
        assert _host(unsupported, parent=False).process_src_audio("x.wav") is None
    assert "format tag 2" in caplog.text

    def never(f):
        raise AssertionError("the native loader ran with the stage off")
    off = _host(never, on=False)
    assert off.process_src_audio("x.wav") == ("parent-src", "x.wav") and off.process_reference_audio(None) == ("parent-ref", None)
    with pytest.raises(RuntimeError, match="no audio input backend"):
        _host(never, parent=False, on=False).process_src_audio("x.wav")
    # the default loader refuses a host without a GPU device instead of computing on the CPU
    from ace355.backend import NativeAudioInMixin
    cpu = type("Host", (NativeAudioInMixin, _Parent), {})()
    cpu.device, cpu.use_native_audio_in = "cpu", True
    assert cpu.process_src_audio(O.wav_bytes(_raw("s16", 2), "s16", 2, 44100))[0] == "parent-src"


def test_op_is_registered_with_a_shape_function():
    from ace355 import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        wav, peak = torch.ops.ace355.audio_in(torch.empty(12048, dtype=torch.uint8, device="cuda"), 44, 1, 2, 3001, 44100)
    assert wav.shape == (2, 3267) and wav.dtype == torch.float32 and peak.shape == (1,)
