"""CPU: the FLAC input path's frame index (ace355_flac_index), its pure plan (csrc/flac_in_plan.h), the ABI structs, the test-side writer
(tests/_flac_streams.py) against the oracle's reader, and the per-frame routines of csrc/flac_in.h run by a stand-alone program under the
host sanitizers (tests/flac_in_host.cpp).  The kernels: tests/test_flac_in_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _flac_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _index(data):
    import ace355  # noqa: F401
    from ace355 import audio_in
    return audio_in.flac_index(data)


# ---------------------------------------------------------------------------------------------------- writer and index
@pytest.mark.parametrize("name", S.STREAMS)
def test_index_matches_the_oracle_walk(name):
    """The writer's samples are what the oracle reads back, and the index's offsets and lengths are the oracle's frame sizes - except on
    the fake-header stream, which has a test of its own."""
    data, rep, pcm, info = S.stream(name)
    assert info["frame_sizes"] == rep["sizes"] and pcm.shape == (sum(rep["blocks"]), info["channels"])
    if name == "fake_header":
        return
    si, table = _index(data)
    assert (si.total_samples, si.channels, si.bits_per_sample, si.sample_rate) == (info["frames"], info["channels"], info["bps"], info["sample_rate"])
    assert (si.min_block, si.max_block, si.first_frame) == (info["min_block"], info["max_block"], rep["offsets"][0])
    assert table[:, 1].tolist() == info["frame_sizes"] and table[:, 0].tolist() == rep["offsets"]
    assert table[:, 3].tolist() == rep["blocks"] and table[:, 2].tolist() == np.concatenate([[0], np.cumsum(rep["blocks"])[:-1]]).tolist()
    assert int(table[-1, 0] + table[-1, 1]) == len(data)


def test_index_reads_long_coded_numbers():
    """Sample numbers past 2^31 take 7 bytes; the header routine reads all UTF-8-style lengths.  (A header alone: no stream is that long.)"""
    for num in (0, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1FFFFF, 0x200000, 0x3FFFFFF, 0x4000000, 0x7FFFFFFF, 0x80000000, (1 << 36) - 1):
        assert len(S.coded_number(num)) == 1 + sum(num >= t for t in (0x80, 0x800, 0x10000, 0x200000, 0x4000000, 0x80000000))


def test_index_accepts_a_byte_exact_fake_header():
    """A verbatim subframe that spells the next frame's header - correct CRC-8, matching fields, the expected next number - is taken for a
    frame boundary: a header walk cannot tell.  This is the residual case the device's CRC-16 exists for (the GPU test shows the fallback)."""
    data, rep, _pcm, info = S.stream("fake_header")
    si, table = _index(data)
    assert len(table) == len(rep["offsets"]) and int(table[:, 3].sum()) == info["frames"]
    assert table[:2, 0].tolist() == rep["offsets"][:2] and int(table[2, 0]) == rep["fake_at"] != rep["offsets"][2]
    assert int(table[1, 1]) < rep["sizes"][1] and table[3:, 0].tolist() == rep["offsets"][3:]


def test_index_refusals():
    z = lambda ch: [dict(samples=np.zeros((16, ch), np.int64), subframes={"kind": "constant"}, bs_code=6) for _ in range(3)]
    cases = {
        "12 bits per sample": S.write_stream(z(1), 1, 12)[0],
        "32 bits per sample": S.write_stream(z(1), 1, 32)[0],
        "max block 32768": S.write_stream(z(1), 1, 16, max_block=32768)[0],
        "max block 15": S.write_stream(z(1), 1, 16, max_block=15)[0],
        "does not say how many samples": S.write_stream(z(1), 1, 16, total=0)[0],
        "sum to 48 samples, STREAMINFO counts 64": S.write_stream(z(1), 1, 16, total=64)[0],
        "hold more samples than STREAMINFO counts": S.write_stream(z(1), 1, 16, total=40)[0],
    }
    three = bytearray(S.write_stream(z(2), 2, 16)[0])
    three[4 + 4 + 12] |= 0x04   # STREAMINFO's channel field (bits 3 .. 1 of this byte): 2 -> 4 channels
    cases["4 channels"] = bytes(three)
    for text, data in cases.items():
        with pytest.raises(NotImplementedError, match=text):
            _index(data)
    with pytest.raises(NotImplementedError, match="not a FLAC stream"):
        _index(b"RIFF" + bytes(64))


def test_index_grows_its_table():
    """More frames than the first table holds: the second call gets the count the first one reported."""
    from ace355 import native
    data = S.stream("many_frames")[0]
    lib, info, n = native.lib(), native.FlacStreamInfoC(), ctypes.c_int64(0)
    buf = np.frombuffer(data, dtype=np.uint8)
    small = np.full((5, 4), -1, dtype=np.int64)
    assert lib.ace355_flac_index(buf.ctypes.data, buf.size, ctypes.byref(info), small.ctypes.data, 4, ctypes.byref(n)) != native.OK
    assert n.value == 2100 and "2100 frames" in native.last_error() and (small[4] == -1).all() and small[3, 2] == 48


# ---------------------------------------------------------------------------------------------------- plan and ABI
def test_plan_values():
    from ace355 import native
    p = native.flac_in_plan(2584, 2, 16, 4096, 240 * 44100)   # 240 s at 4096-sample blocks
    total = 240 * 44100
    assert p["launches"] == 4 and (p["entropy_threads"], p["restore_threads"], p["finish_threads"], p["status_threads"]) == (64, 64, 256, 256)
    assert (p["entropy_lanes"], p["entropy_grid"]) == (3, 862) and (p["restore_lanes"], p["restore_grid"]) == (6, 862)
    assert (p["finish_tiles"], p["finish_grid"]) == (16, 2584 * 16)
    assert p["desc_at"] == 8 * total and p["frame_at"] == 8 * total + 2584 * 320 and p["scratch_bytes"] == 8 * total + 2584 * 328
    assert p["out_format"] == "s16" and p["out_bytes"] == 4 * total
    p = native.flac_in_plan(323, 1, 24, 4096, 30 * 44100 + 1)     # 30 s mono at 24 bits: a wave per frame
    assert (p["entropy_lanes"], p["entropy_grid"], p["restore_lanes"], p["restore_grid"]) == (1, 323, 1, 323)
    assert p["out_format"] == "s32" and p["out_bytes"] == 4 * (30 * 44100 + 1) and p["desc_at"] == (4 * (30 * 44100 + 1) + 15) // 16 * 16
    p = native.flac_in_plan(3, 1, 16, 16, 33)                     # odd mono int16 output: padded to a multiple of 4
    assert p["out_bytes"] == 68 and p["finish_tiles"] == 1 and p["finish_grid"] == 3
    p = native.flac_in_plan(1 << 24, 2, 17, 16384, 1 << 32)       # the largest table: 64 lanes per wave
    assert (p["entropy_lanes"], p["entropy_grid"], p["restore_lanes"], p["restore_grid"]) == (64, 1 << 18, 64, 1 << 19)
    assert p["finish_grid"] == (1 << 24) * 64 and p["out_format"] == "s32"
    assert native.flac_in_plan(1025, 1, 16, 4096, 4096 * 1025)["entropy_lanes"] == 2 and native.flac_in_plan(1024, 1, 16, 4096, 4096 * 1024)["entropy_lanes"] == 1


@pytest.mark.parametrize("args, text", [((0, 2, 16, 4096, 100), "frames"), (((1 << 24) + 1, 2, 16, 4096, 1 << 30), "frames"), ((10, 3, 16, 4096, 100), "channels"),
                                        ((10, 0, 16, 4096, 100), "channels"), ((10, 2, 15, 4096, 100), "bits"), ((10, 2, 25, 4096, 100), "bits"),
                                        ((10, 2, 16, 15, 100), "max block"), ((10, 2, 16, 16385, 100), "max block"), ((10, 2, 16, 4096, 0), "total"),
                                        ((10, 2, 16, 4096, (1 << 32) + 1), "total"), ((10, 2, 16, 4096, 9), "cannot hold"), ((10, 2, 16, 4096, 40961), "cannot hold")])
def test_plan_refusals(args, text):
    from ace355 import native
    with pytest.raises(RuntimeError, match=text):
        native.flac_in_plan(*args)


def test_struct_layouts_match_header(tmp_path):
    from ace355 import native
    structs = {"ace355_flac_stream_info": native.FlacStreamInfoC, "ace355_flac_in_plan_info": native.FlacInPlanInfoC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _t in ct._fields_]
    lines += [f'  printf("status {i} %d\\n", {c});' for i, c in enumerate(("ACE355_FLAC_OK", "ACE355_FLAC_HEADER_MISMATCH", "ACE355_FLAC_RESERVED",
                                                                        "ACE355_FLAC_OVERRUN", "ACE355_FLAC_SAMPLE_COUNT", "ACE355_FLAC_CRC16"))]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    sizes = {l[0]: int(l[1]) for l in got if len(l) == 2}
    for cname, ct in structs.items():
        assert sizes[cname] == ctypes.sizeof(ct), cname
        for fname, _t in ct._fields_:
            assert sizes[f"{cname}.{fname}"] == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(l[2]) for l in got if l[0] == "status"] == list(range(len(native.FLAC_STATUS)))


def test_flag_defaults_off():
    import inspect
    from ace355 import audio_in
    from ace355.backend import NativeAudioInMixin
    assert inspect.signature(audio_in.load_stereo_48k).parameters["flac_on_gpu"].default is False
    assert NativeAudioInMixin.native_flac_decode is (os.environ.get("ACE355_FLAC_GPU", "") == "1")


# ---------------------------------------------------------------------------------------------------- the stand-alone program
def _case_file(path, name):
    data, _rep, pcm, info = S.stream(name)
    si, table = _index(data)
    head = np.array([si.channels, si.bits_per_sample, si.sample_rate, si.variable_blocks, si.total_samples, len(table), si.max_block, len(data)], dtype="<i8")
    with open(path, "wb") as f:
        f.write(head.tobytes() + table.astype("<i8").tobytes() + pcm.astype("<i8").tobytes() + data)


def test_frame_routines_under_host_sanitizers(tmp_path):
    """csrc/flac_in.h on the CPU, as the kernels call it: every stream decodes to the oracle's samples (the fake-header stream apart: its
    table is wrong by construction); 2000 seeded single-bit and single-byte corruptions of the small streams leave every frame with
    "status != ok, or the oracle's samples", and neither run draws a sanitizer report."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "flac_in_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "flac_in_host.cpp"), "-o", str(exe)], check=True)
    files = {}
    for name in S.STREAMS:
        files[name] = str(tmp_path / f"{name}.case")
        _case_file(files[name], name)
    r = subprocess.run([str(exe), "decode"] + [files[n] for n in S.STREAMS if n != "fake_header"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    assert r.stdout.count(": equal") == len(S.STREAMS) - 1
    bad = subprocess.run([str(exe), "decode", files["fake_header"]], capture_output=True, text=True)
    assert bad.returncode == 1 and "frame 1 status 3" in bad.stderr, bad.stderr[-2000:]   # the split frame runs past its range
    r = subprocess.run([str(exe), "corrupt", "2000", "1"] + [files[n] for n in S.SMALL if n != "fake_header"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    assert "ok with wrong samples 0" in r.stdout
    print(r.stdout)
