"""Test-side FLAC writer (RFC 9639) driven by a per-frame spec, and the streams the FLAC input tests share.

``oracle.audio_out.flac_encode_test_stream`` writes 16-bit independent-channel LPC streams only; the GPU decode (csrc/flac_in.hip) has to
be shown every subframe form at 16, 20 and 24 bits.  ``write_stream`` takes, per frame: the samples, the channel assignment, the header's
block-size code where two are legal, and per subframe the kind / order / precision / shift / coefficients / Rice method / partition
order / fixed Rice parameter / which partitions are escaped and with how many raw bits / wasted bits.  It reports the largest
``|sum coef * sample|`` it produced.  ``oracle.audio_out.flac_decode`` is the independent reader: ``stream(name)`` returns its samples.

Every stream stays at or under about 40 000 samples so that the pure-Python writer and reader take a second or two.
"""
from __future__ import annotations

import hashlib
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def _table(poly: int, width: int) -> List[int]:
    top, mask, out = 1 << (width - 1), (1 << width) - 1, []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


class BitWriter:
    def __init__(self):
        self.parts: List[str] = []

    def put(self, v: int, n: int):
        if n:
            self.parts.append(format(int(v) & ((1 << n) - 1), f"0{n}b"))

    def unary(self, q: int):
        self.parts.append("0" * int(q) + "1")

    def tobytes(self) -> bytes:
        bits = "".join(self.parts)
        bits += "0" * (-len(bits) % 8)
        return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def coded_number(num: int) -> bytes:
    """The UTF-8-style number of a frame header: 1 to 7 bytes, up to 36 bits."""
    if num < 0x80:
        return bytes([num])
    nb = 2
    while nb < 7 and num >> (5 * nb + 1):
        nb += 1
    out = [((0xFF00 >> nb) & 0xFF) | (num >> (6 * (nb - 1)))]
    out += [0x80 | ((num >> (6 * i)) & 0x3F) for i in range(nb - 2, -1, -1)]
    return bytes(out)


def frame_header(block: int, number: int, assign: int, bps: int, sample_rate: int, variable: bool, bs_code: Optional[int] = None) -> bytes:
    """A frame header with its CRC-8.  ``bs_code``: the block-size code to use where more than one is legal (6: 8-bit field, 7: 16-bit
    field, else the code that names the size); None: the named code when there is one, else the shorter field."""
    if bs_code is None:
        bs_code = BS_CODES.get(block) or (6 if block <= 256 else 7)
    assert (bs_code == 6 and block <= 256) or (bs_code == 7 and block <= 65536) or BS_CODES.get(block) == bs_code
    h = bytes([0xFF, 0xF8 | (1 if variable else 0), (bs_code << 4) | SR_CODES.get(sample_rate, 0), (assign << 4) | (SS_CODES.get(bps, 0) << 1)])
    h += coded_number(number)
    if bs_code == 6:
        h += bytes([block - 1])
    elif bs_code == 7:
        h += (block - 1).to_bytes(2, "big")
    return h + bytes([crc8(h)])


def _raw_bits(r: np.ndarray) -> int:
    """The fewest bits that hold every value of r in two's complement; 0 when all are zero."""
    if r.size == 0 or not r.any():
        return 0
    return max(int(v).bit_length() for v in (int(r.max()), -int(r.min()) - 1, 0)) + 1


def _subframe(bw: BitWriter, sig: np.ndarray, bps: int, spec: Dict, report: Dict):
    n, kind, w = len(sig), spec.get("kind", "verbatim"), int(spec.get("wasted", 0))
    sig = sig.astype(np.int64)
    if w:
        assert not (sig & ((1 << w) - 1)).any(), "wasted bits need samples that are multiples of 2^w"
        sig, bps = sig >> w, bps - w
    assert -(1 << (bps - 1)) <= int(sig.min()) and int(sig.max()) < (1 << (bps - 1)), "sample outside the subframe's bit depth"
    order = int(spec.get("order", 0))
    typ = {"constant": 0, "verbatim": 1, "fixed": 8 | order, "lpc": 32 | (order - 1)}[kind]
    bw.put(0, 1), bw.put(typ, 6)
    if w:
        bw.put(1, 1), bw.unary(w - 1)
    else:
        bw.put(0, 1)
    if kind == "constant":
        assert (sig == sig[0]).all()
        return bw.put(int(sig[0]), bps)
    if kind == "verbatim":
        for v in sig:
            bw.put(int(v), bps)
        return None
    assert order <= n
    for v in sig[:order]:
        bw.put(int(v), bps)
    if kind == "lpc":
        prec, shift = int(spec["precision"]), int(spec["shift"])
        X = np.stack([sig[order - 1 - k:n - 1 - k] for k in range(order)], 1) if n > order else np.zeros((0, order), np.int64)
        if "coefs" in spec:
            q = np.asarray(spec["coefs"], dtype=np.int64)
        else:   # least squares on this block, quantised with the given shift
            c = np.linalg.lstsq(X.astype(np.float64), sig[order:].astype(np.float64), rcond=None)[0] if n > order else np.zeros(order)
            q = np.clip(np.rint(c * (1 << shift)), 1 - (1 << (prec - 1)), (1 << (prec - 1)) - 1).astype(np.int64)
        assert len(q) == order and int(np.abs(q).max(initial=0)) < (1 << (prec - 1))
        bw.put(prec - 1, 4), bw.put(shift, 5)
        for v in q:
            bw.put(int(v), prec)
        sums = X @ q
        report["max_pred_sum"] = max(report["max_pred_sum"], int(np.abs(sums).max(initial=0)))
        res = sig[order:] - (sums >> shift)
    else:
        q = np.asarray(FIXED[order], dtype=np.int64)
        X = np.stack([sig[order - 1 - k:n - 1 - k] for k in range(order)], 1) if order and n > order else np.zeros((max(n - order, 0), 0), np.int64)
        res = sig[order:] - (X @ q if order else 0)
    assert int(np.abs(res).max(initial=0)) < (1 << 31), "residual outside int32"
    method, po = int(spec.get("method", 0)), int(spec.get("partition_order", 0))
    kbits, esc = (4, 15) if method == 0 else (5, 31)
    assert po == 0 or (n % (1 << po) == 0 and (n >> po) >= order)
    bw.put(method, 2), bw.put(po, 4)
    escapes, plen, at = spec.get("escapes", {}), n >> po, 0
    for p in range(1 << po):
        cnt = plen - (order if p == 0 else 0)
        r = res[at:at + cnt]
        at += cnt
        if p in escapes:
            raw = _raw_bits(r) if escapes[p] is None else int(escapes[p])
            assert raw >= _raw_bits(r) and raw <= 31
            bw.put(esc, kbits), bw.put(raw, 5)
            for v in r:
                bw.put(int(v), raw)
            continue
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        k = spec.get("k")
        if k is None:
            k = min(max(int(np.log2(max(float(u.mean()) if cnt else 1.0, 1.0))), 0), esc - 1)
        assert 0 <= k < esc
        bw.put(k, kbits)
        for v in u:
            v = int(v)
            bw.unary(v >> k), bw.put(v, k)
    return None


def write_stream(frames: Sequence[Dict], channels: int, bps: int, sample_rate: int = 44100, variable: bool = False,
                 total: Optional[int] = None, max_block: Optional[int] = None) -> Tuple[bytes, Dict]:
    """frames: dicts with ``samples`` int [n, channels], ``assign`` (0 / 1 independent, 8 left/side, 9 side/right, 10 mid/side; default
    independent), ``bs_code`` (optional), ``subframes`` (one spec per channel, or one for all).  ``variable``: sample-number headers.
    ``total`` / ``max_block`` override what STREAMINFO says.  -> (the stream, {"max_pred_sum", "offsets", "sizes", "blocks"})."""
    report = {"max_pred_sum": 0, "offsets": [], "sizes": [], "blocks": []}
    body, pos, pcm = bytearray(), 0, []
    for fno, fr in enumerate(frames):
        x = np.asarray(fr["samples"], dtype=np.int64).reshape(-1, channels)
        n, assign = len(x), int(fr.get("assign", channels - 1))
        assert (assign == channels - 1) or (channels == 2 and assign in (8, 9, 10))
        if assign == 8:
            sigs, side = [x[:, 0], x[:, 0] - x[:, 1]], (False, True)
        elif assign == 9:
            sigs, side = [x[:, 0] - x[:, 1], x[:, 1]], (True, False)
        elif assign == 10:
            sigs, side = [(x[:, 0] + x[:, 1]) >> 1, x[:, 0] - x[:, 1]], (False, True)
        else:
            sigs, side = [x[:, c] for c in range(channels)], (False,) * channels
        bw = BitWriter()
        subs = fr.get("subframes", {"kind": "verbatim"})
        for c in range(channels):
            _subframe(bw, sigs[c], bps + (1 if side[c] else 0), subs if isinstance(subs, dict) else subs[c], report)
        frame = frame_header(n, pos if variable else fno, assign, bps, sample_rate, variable, fr.get("bs_code")) + bw.tobytes()
        frame += crc16(frame).to_bytes(2, "big")
        report["offsets"].append(len(body)), report["sizes"].append(len(frame)), report["blocks"].append(n)
        body += frame
        pos += n
        pcm.append(x)
    allpcm = np.concatenate(pcm, 0)
    blocks = report["blocks"]
    si = BitWriter()
    si.put(min(blocks[:-1] or blocks), 16), si.put(max(blocks) if max_block is None else max_block, 16), si.put(0, 24), si.put(0, 24)
    si.put(sample_rate, 20), si.put(channels - 1, 3), si.put(bps - 1, 5), si.put(pos if total is None else total, 36)
    md5 = hashlib.md5(allpcm.astype("<i2").tobytes()).digest() if bps == 16 else bytes(16)
    head = b"fLaC" + bytes([0x80, 0, 0, 34]) + si.tobytes() + md5
    report["offsets"] = [o + len(head) for o in report["offsets"]]
    return head + bytes(body), report


# ---------------------------------------------------------------------------------------------------- the shared streams
def _noise(rng, n: int, channels: int, bits: int) -> np.ndarray:
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(n, channels), dtype=np.int64)


def _tones(n: int, channels: int, bps: int, seed: int, noise_bits: int = 4) -> np.ndarray:
    """Something a predictor has a grip on: two sines per channel plus a little noise, about a quarter of full scale."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None]
    f = rng.uniform(0.01, 0.2, size=(2, channels))
    x = (np.sin(t * f[0]) + 0.5 * np.sin(t * f[1] + 1.0)) * (1 << (bps - 3))
    return np.rint(x).astype(np.int64) + _noise(rng, n, channels, noise_bits)


def _cut(x: np.ndarray, blocks: Sequence[int], specs) -> List[Dict]:
    """Frames of the given block sizes over x; specs: one dict of frame fields for all, or a function of the frame index."""
    out, at = [], 0
    for i, b in enumerate(blocks):
        fr = dict(specs(i) if callable(specs) else specs)
        fr["samples"] = x[at:at + b]
        out.append(fr)
        at += b
    assert at == len(x)
    return out


def _fake_header_stream() -> Tuple[bytes, Dict]:
    """Mono, 16 bits, 16-sample frames with frame-number headers.  Frame 1 is verbatim and four of its samples spell, byte for byte, the
    header frame 2 would have: correct CRC-8, matching fields, the expected next number.  A header walk accepts it."""
    x = _tones(16 * 6, 1, 16, seed=41)
    fake = frame_header(16, 2, 0, 16, 44100, False, bs_code=6)
    assert len(fake) == 7
    fake += b"\x00"
    x[16 + 6:16 + 10, 0] = np.frombuffer(fake, dtype=">i2")
    frames = _cut(x, [16] * 6, lambda i: {"bs_code": 6, "subframes": {"kind": "verbatim"} if i == 1 else {"kind": "fixed", "order": 1}})
    data, rep = write_stream(frames, 1, 16)
    rep["fake_at"] = rep["offsets"][1] + 7 + 1 + 2 * 6   # frame header, subframe header byte, six samples
    assert data[rep["fake_at"]:rep["fake_at"] + 7] == fake[:7]
    return data, rep


def _build(name: str) -> Tuple[bytes, Dict]:
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("one_frame_"):
        kind = name[len("one_frame_"):]
        x = np.full((16, 1), -1234, dtype=np.int64) if kind == "constant" else _tones(16, 1, 16, seed=3)
        sub = {"constant": {"kind": "constant"}, "verbatim": {"kind": "verbatim"}, "fixed": {"kind": "fixed", "order": 2},
               "lpc": {"kind": "lpc", "order": 3, "precision": 10, "shift": 8}}[kind]
        return write_stream(_cut(x, [16], {"subframes": sub, "bs_code": 6}), 1, 16)
    if name == "wave_boundary":   # 70 frames: lanes / waves past 64, the four channel assignments cycling
        x = _tones(70 * 192, 2, 16, seed=5)
        return write_stream(_cut(x, [192] * 70, lambda i: {"assign": (1, 8, 9, 10)[i % 4], "subframes": {"kind": "fixed", "order": 2, "partition_order": 2}}), 2, 16)
    if name == "many_frames":     # frame numbers 0 .. 2099: 1-, 2- and 3-byte coded numbers
        x = _tones(2100 * 16, 1, 16, seed=6)
        return write_stream(_cut(x, [16] * 2100, {"bs_code": 6, "subframes": {"kind": "fixed", "order": 1}}), 1, 16)
    if name == "many_frames_variable":   # the same samples, sample-number headers, blocks 16 / 32 / 64
        x = _tones(2100 * 16, 1, 16, seed=6)
        return write_stream(_cut(x, [16, 32, 64] * 300, {"bs_code": 6, "subframes": {"kind": "fixed", "order": 1}}), 1, 16, variable=True)
    if name == "block_codes":     # every named size the GPU decode takes, then a short block through the 8-bit field
        blocks = [192, 576, 1152, 4096, 4608, 100]
        x = _tones(sum(blocks), 2, 16, seed=7)
        return write_stream(_cut(x, blocks, lambda i: {"assign": 10, "bs_code": 6 if i == 5 else None, "subframes": {"kind": "fixed", "order": 2, "partition_order": 2 if i < 5 else 0}}),
                            2, 16, variable=True)
    if name == "short_last_16bit_field":   # fixed blocking: the last block is short and goes through the 16-bit field
        blocks = [4096, 4096, 1000]
        x = _tones(sum(blocks), 1, 16, seed=8)
        return write_stream(_cut(x, blocks, lambda i: {"bs_code": 7 if i == 2 else None, "subframes": {"kind": "fixed", "order": 3, "partition_order": 3}}), 1, 16)
    if name == "fixed_orders":
        x = _tones(5 * 256, 1, 16, seed=9)
        return write_stream(_cut(x, [256] * 5, lambda i: {"subframes": {"kind": "fixed", "order": i, "partition_order": 4}}), 1, 16)
    if name == "lpc":             # orders 1, 8, 12, 32 at precision 12; precision 15 with shift 0 and with shift 14
        x = _tones(6 * 256, 1, 16, seed=10, noise_bits=8)
        subs = [{"kind": "lpc", "order": o, "precision": 12, "shift": 9, "partition_order": 2} for o in (1, 8, 12, 32)]
        subs.append({"kind": "lpc", "order": 2, "precision": 15, "shift": 0, "coefs": [2, -1]})
        subs.append({"kind": "lpc", "order": 2, "precision": 15, "shift": 14, "coefs": [16383, -8192]})
        return write_stream(_cut(x, [256] * 6, lambda i: {"subframes": subs[i]}), 1, 16)
    if name == "rice":            # k = 0, k = 14 (the last 4-bit parameter), Rice2 with k = 15 and k = 17
        small = np.cumsum(rng.integers(-1, 2, size=(256, 1)), 0)
        loud = _noise(rng, 256 * 3, 1, 16)
        x = np.concatenate([small, loud], 0)
        subs = [{"kind": "fixed", "order": 1, "k": 0}, {"kind": "fixed", "order": 0, "k": 14}, {"kind": "fixed", "order": 1, "method": 1, "k": 15},
                {"kind": "fixed", "order": 2, "method": 1, "k": 17, "partition_order": 3}]
        return write_stream(_cut(x, [256] * 4, lambda i: {"subframes": subs[i]}), 1, 16)
    if name == "partitions":      # order 0 and the largest a 256-sample block allows (8: one sample each, none in partition 0); 0 raw bits
        x = _tones(3 * 256, 1, 16, seed=12)
        x[512:] = 777                                   # fixed order 1 on a constant: every residual is zero
        subs = [{"kind": "fixed", "order": 2, "partition_order": 0}, {"kind": "fixed", "order": 1, "partition_order": 8},
                {"kind": "fixed", "order": 1, "partition_order": 2, "escapes": {0: 0, 2: 0, 3: 5}}]
        return write_stream(_cut(x, [256] * 3, lambda i: {"subframes": subs[i]}), 1, 16)
    if name == "escape_25_bits":  # 24 bits, left/side: the side channel is 25 bits and full scale, escaped at its full width
        x = _noise(rng, 2 * 128, 2, 24)
        x[0] = (-(1 << 23), (1 << 23) - 1)              # side = -2^24 + 1 ... and the other extreme below
        x[1] = ((1 << 23) - 1, -(1 << 23))
        sub = {"kind": "fixed", "order": 0, "partition_order": 1, "escapes": {0: 25, 1: None}}
        return write_stream(_cut(x, [128] * 2, {"assign": 8, "subframes": [{"kind": "verbatim"}, sub]}), 2, 24)
    if name == "wasted":          # wasted bits 1 and 7
        x = _tones(2 * 256, 1, 16, seed=13)
        x[:256] &= ~1
        x[256:] &= ~127
        subs = [{"kind": "lpc", "order": 4, "precision": 12, "shift": 9, "wasted": 1}, {"kind": "fixed", "order": 2, "wasted": 7}]
        return write_stream(_cut(x, [256] * 2, lambda i: {"subframes": subs[i]}), 1, 16)
    if name == "ms24":            # 24 bits, full-scale noise, mid/side, LPC order 32 at precision 15: prediction sums past 2^31
        x = _noise(rng, 2 * 512, 2, 24)
        coefs = [int(v) for v in rng.integers(-16383, 16384, size=32)]
        sub = {"kind": "lpc", "order": 32, "precision": 15, "shift": 14, "coefs": coefs, "method": 1, "partition_order": 3}
        return write_stream(_cut(x, [512] * 2, {"assign": 10, "subframes": sub}), 2, 24)
    if name == "bps20":
        x = _tones(3 * 512, 2, 20, seed=14)
        return write_stream(_cut(x, [512] * 3, lambda i: {"assign": (10, 8, 1)[i], "subframes": {"kind": "lpc", "order": 8, "precision": 13, "shift": 10, "partition_order": 2}}), 2, 20)
    if name in ("e2e_44k", "e2e_48k", "e2e24_44k"):
        bps, rate = (24 if "24" in name else 16), (48000 if "48k" in name else 44100)
        x = _tones(3 * 1152 + 300, 2, bps, seed=15)
        return write_stream(_cut(x, [1152] * 3 + [300], lambda i: {"assign": 10, "subframes": {"kind": "lpc", "order": 8, "precision": 12, "shift": 9, "partition_order": 2}}),
                            2, bps, sample_rate=rate)
    if name in ("verbatim16", "verbatim24"):   # bits that carry nothing but a sample: a flipped one changes the CRC-16 and nothing else
        bps = int(name[-2:])
        x = _noise(rng, 3 * 64 + 5, 2, bps)
        return write_stream(_cut(x, [64] * 3 + [5], {"bs_code": 6, "subframes": {"kind": "verbatim"}}), 2, bps)
    if name == "fake_header":
        return _fake_header_stream()
    raise KeyError(name)


ONE_FRAME = ("one_frame_constant", "one_frame_verbatim", "one_frame_fixed", "one_frame_lpc")
# name -> what it covers (the rows of the GPU test table)
STREAMS = ONE_FRAME + ("wave_boundary", "many_frames", "many_frames_variable", "block_codes", "short_last_16bit_field", "fixed_orders", "lpc",
                       "rice", "partitions", "escape_25_bits", "wasted", "ms24", "bps20", "e2e_44k", "e2e_48k", "e2e24_44k", "verbatim16", "verbatim24",
                       "fake_header")
SMALL = ONE_FRAME + ("fixed_orders", "lpc", "rice", "partitions", "escape_25_bits", "wasted", "ms24", "bps20", "fake_header")   # for the corruption sweep


@lru_cache(maxsize=None)
def stream(name: str) -> Tuple[bytes, Dict, np.ndarray, Dict]:
    """(the stream, the writer's report, the oracle's samples int64 [total, channels], the oracle's info) - computed once per process."""
    from oracle import audio_out as o_out
    data, rep = _build(name)
    pcm, info = o_out.flac_decode(data)
    pcm.setflags(write=False)
    return data, rep, pcm, info
