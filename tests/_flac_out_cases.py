"""The inputs of the FLAC output tests (tests/test_flac_out_cpu.py, tests/test_flac_out_gpu.py): the 13 signals of tests/test_audio_out.py
(the same recipe) plus five that reach the encoder choices those leave out, the long cases for 2- and 3-byte frame numbers, the sample
rates of the five header forms, and a reader of the choices a stream made (from the host encoder's bytes)."""
import functools

import numpy as np

N = 4096 * 2 + 1234
RATES = (44100, 32000, 12000, 12345, 123450)   # table / kHz byte / Hz word / tens-of-Hz word (700001, STREAMINFO only, is below)


def _to16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def signals():
    rng = np.random.default_rng(5)
    n = N
    t = np.arange(n) / 48000.0
    sine = np.stack([0.6 * np.sin(2 * np.pi * 220 * t), 0.55 * np.sin(2 * np.pi * 220 * t + 0.1) + 0.05 * np.sin(2 * np.pi * 3000 * t)], 1)
    music = np.cumsum(rng.standard_normal((n, 2)) * 0.01, 0)
    music[:, 1] = 0.9 * music[:, 0] + 0.02 * rng.standard_normal(n)
    sq = np.where((np.arange(n) // 7) % 2 == 0, 32767, -32768)[:, None].repeat(2, 1).astype(np.int16)
    to16 = lambda x: _to16(x * 32767)  # noqa: E731
    out = {
        "sine_stereo": to16(sine), "walk_stereo": to16(music / np.abs(music).max()), "noise_stereo": to16(rng.uniform(-1, 1, (n, 2))),
        "silence": np.zeros((n, 2), np.int16), "dc": np.full((5000, 2), -1234, np.int16), "square_extremes": sq,
        "mono_sine": to16(sine[:, :1]), "one_sample": np.array([[7, -9]], np.int16), "short": to16(sine[:5]),
        "exact_block": to16(sine[:4096]), "tiny_tail": to16(sine[:4096 + 3]), "right_only": np.stack([np.zeros(n, np.int16), to16(sine[:, 0])], 1),
        "left_plus_small": np.stack([to16(sine[:, 0]), (to16(sine[:, 0]).astype(np.int32) + rng.integers(-2, 3, n)).clip(-32768, 32767).astype(np.int16)], 1),
    }
    # the five additions
    rng = np.random.default_rng(11)
    s = 19000 * np.sin(2 * np.pi * 220 * t)
    out["small_plus_right"] = np.stack([_to16(s + rng.integers(-2, 3, n)), _to16(s)], 1)
    A, B = 15000 * np.sin(2 * np.pi * 180 * t), rng.integers(-100, 101, n)
    out["mid_side"] = np.stack([_to16(A + B), _to16(A - B)], 1)
    amp = np.where((np.arange(n) // 16) % 2 == 0, 2, 2000)
    out["bursts16"] = np.stack([_to16(rng.integers(-1, 2, n) * amp * rng.random(n)), _to16(rng.integers(-1, 2, n) * amp[::-1] * rng.random(n))], 1)
    out["loud_noise"] = np.stack([_to16(rng.integers(-2000, 2001, n)), _to16(rng.integers(-2000, 2001, n))], 1)
    click = s.copy()
    click[500::1000] += 12000
    out["clicks"] = np.stack([_to16(click), _to16(s)], 1)
    return out


ORIGINAL = ("sine_stereo", "walk_stereo", "noise_stereo", "silence", "dc", "square_extremes", "mono_sine", "one_sample", "short", "exact_block",
            "tiny_tail", "right_only", "left_plus_small")
ADDED = ("small_plus_right", "mid_side", "bursts16", "loud_noise", "clicks")
BATCH3 = ("sine_stereo", "mid_side", "bursts16")   # equal length, different content


@functools.lru_cache(maxsize=None)
def long_cases():
    """129 blocks of stereo (2-byte frame numbers from frame 128 on) and 2049 blocks of mono, silent but for the last three (3-byte frame
    numbers from frame 2048 on; a 240 s song has 2813 blocks)."""
    rng = np.random.default_rng(12)
    n = 4096 * 128 + 777
    t = np.arange(n) / 48000.0
    x = 9000 * np.sin(2 * np.pi * 330 * t) * (1 + 0.3 * np.sin(2 * np.pi * 0.5 * t)) + rng.integers(-40, 41, n)
    blocks129 = np.stack([_to16(x), _to16(0.8 * x + rng.integers(-40, 41, n))], 1)
    n = 4096 * 2048 + 100
    mono = np.zeros((n, 1), np.int16)
    tail = n - (4096 * 2046)
    mono[-tail:, 0] = _to16(7000 * np.sin(2 * np.pi * 440 * np.arange(tail) / 48000.0) + rng.integers(-5, 6, tail))
    return {"blocks129": blocks129, "blocks2049_mono": mono}


@functools.lru_cache(maxsize=None)
def host_bytes(name, sample_rate=48000):
    """The host encoder's stream of a case: the reference of every comparison, computed once."""
    from ace355 import audio_out
    return audio_out.flac_encode_pcm16(pcm_of(name), sample_rate, n_threads=4)


def pcm_of(name):
    if name in signals():
        return signals()[name]
    if name == "empty":
        return np.zeros((0, 2), np.int16)
    if name == "rates":
        return signals()["sine_stereo"][:3000]
    return long_cases()[name]


def frame_starts(data):
    """Byte offset of every frame of a stream, from the oracle reader's frame sizes."""
    from oracle import audio_out as o_audio
    _pcm, info = o_audio.flac_decode(data)
    at, out = 42, []
    for sz in info["frame_sizes"]:
        out.append(at)
        at += sz
    assert at == len(data)
    return out


def assignments(data):
    """The channel-assignment nibbles (byte 3 of each frame header) a stream uses."""
    return sorted({data[at + 3] >> 4 for at in frame_starts(data)})


def coded_number_bytes(data):
    """The longest coded frame number of a stream, in bytes."""
    best = 0
    for at in frame_starts(data):
        lead, nb = data[at + 4], 0
        while lead & (0x80 >> nb):
            nb += 1
        best = max(best, nb or 1)
    return best
