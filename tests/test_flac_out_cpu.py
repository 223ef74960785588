"""CPU: the FLAC output path's pure plan (csrc/flac_out_plan.h), its ABI structs, the STREAMINFO routine, the coverage the inputs of
tests/_flac_out_cases.py reach on the HOST encoder, and the per-frame routines of csrc/flac_out.h run by a stand-alone program under the host
sanitizers (tests/flac_out_host.cpp) against the host encoder's bytes.  The kernels: tests/test_flac_out_gpu.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _flac_out_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 4096 * 2 * 17 // 8 + 64


def _bound(frames, ch):
    nblk = (frames + 4095) // 4096
    return 42 + nblk * 32 + (frames * ch * 17 + 7) // 8 + nblk * ch * 2


# ---------------------------------------------------------------------------------------------------- plan and ABI
@pytest.mark.parametrize("n_items, frames, ch", [(8, 30 * 48000, 2), (8, 240 * 48000, 2), (1, 1, 1), (4096, 512 * 4096, 2), (1, (1 << 21) * 4096, 1)])
def test_plan_values(n_items, frames, ch):
    import ace355  # noqa: F401
    from ace355 import native
    p = native.flac_out_plan(n_items, frames, ch)
    blocks = (frames + 4095) // 4096
    units = blocks * n_items
    assert (p["launches"], p["blocks"], p["units"]) == (3, blocks, units)
    assert (p["frame_grid"], p["offsets_grid"], p["gather_grid"]) == (units, n_items, units)
    assert (p["frame_threads"], p["offsets_threads"], p["gather_threads"]) == (256, 256, 256)
    assert p["slot_stride"] == SLOT == 17472 and 50 * 1024 < p["frame_lds_bytes"] <= 64 * 1024   # at least two workgroups in a CU's 160 KiB
    assert p["item_stride"] == (_bound(frames, ch) + 15) // 16 * 16 == (int(native.lib().ace355_flac_bound(frames, ch)) + 15) // 16 * 16
    assert p["out_bytes"] == n_items * p["item_stride"] and p["records_bytes"] == 32 * n_items
    assert p["sizes_at"] == units * SLOT and p["offsets_at"] == (p["sizes_at"] + 4 * units + 15) // 16 * 16
    assert p["scratch_bytes"] == p["offsets_at"] + 8 * units and p["scratch_bytes"] < 1 << 36
    if (n_items, frames) == (8, 30 * 48000):
        assert (blocks, units) == (352, 2816) and p["scratch_bytes"] == 2816 * (17472 + 4 + 8)


@pytest.mark.parametrize("args, text", [((0, 100, 2), "n_items"), ((4097, 100, 2), "n_items"), ((1, 100, 0), "channels"), ((1, 100, 3), "channels"),
                                        ((1, 0, 2), "frames"), ((1, -1, 2), "frames"), ((1, 1 << 36, 2), "frames"), ((4096, 512 * 4096 + 1, 1), "n_items x blocks"),
                                        ((1, (1 << 21) * 4096 + 1, 1), "n_items x blocks")])
def test_plan_refusals(args, text):
    from ace355 import native
    with pytest.raises(RuntimeError, match=text):
        native.flac_out_plan(*args)


def test_struct_layouts_match_header(tmp_path):
    from ace355 import native
    structs = {"ace355_flac_out_plan_info": native.FlacOutPlanInfoC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _t in ct._fields_]
    lines += ['  printf("flags %u %u\\n", ACE355_SAVE_FLAC_GPU, ACE355_SAVE_FLAC_NO_MD5);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    sizes = {l[0]: int(l[1]) for l in got if len(l) == 2}
    for cname, ct in structs.items():
        assert sizes[cname] == ctypes.sizeof(ct), cname
        for fname, _t in ct._fields_:
            assert sizes[f"{cname}.{fname}"] == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [l[1:] for l in got if l[0] == "flags"] == [[str(native.SAVE_FLAC_GPU), str(native.SAVE_FLAC_NO_MD5)]]


def test_flag_defaults_off():
    import inspect
    from ace355 import audio_out
    assert inspect.signature(audio_out.AudioSaver.__init__).parameters["flac_on_gpu"].default is None
    assert audio_out.FLAC_OUT_GPU_DEFAULT is (os.environ.get("ACE355_FLAC_OUT_GPU", "") == "1")
    s = audio_out.AudioSaver()
    assert s.flac_on_gpu is audio_out.FLAC_OUT_GPU_DEFAULT and s.flac_md5 is True and s.last_flac_report is None
    assert audio_out.AudioSaver(flac_on_gpu=True, flac_md5=False).flac_on_gpu is True


# ---------------------------------------------------------------------------------------------------- STREAMINFO
@pytest.mark.parametrize("name, sr", [("sine_stereo", 48000), ("mono_sine", 48000), ("one_sample", 48000), ("empty", 48000), ("rates", 12345), ("rates", 700001)])
def test_streaminfo_equals_the_host_encoder(name, sr):
    from ace355 import native
    from oracle import audio_out as o_audio
    data, pcm = K.host_bytes(name, sr), K.pcm_of(name)
    sizes = o_audio.flac_decode(data)[1]["frame_sizes"] if sr != 700001 else None   # (the oracle reader has no rate for "see STREAMINFO")
    mn, mx = (min(sizes), max(sizes)) if sizes else (0, 0) if sizes is not None else (int.from_bytes(data[12:15], "big"), int.from_bytes(data[15:18], "big"))
    assert native.flac_streaminfo(pcm.shape[0], pcm.shape[1], sr, mn, mx, data[26:42]) == data[:42]
    assert native.flac_streaminfo(pcm.shape[0], pcm.shape[1], sr, mn, mx) == data[:26] + bytes(16)


# ---------------------------------------------------------------------------------------------------- what the inputs reach, on the host encoder
def test_inputs_reach_every_assignment_and_number_length():
    """The conditions the kernel tests rely on, asserted on the HOST encoder's bytes: the 13 original signals use assignments 1 and 8 (and
    mono's 0) only, the five additions bring in 9 and 10; the long cases reach 2- and 3-byte coded frame numbers."""
    seen = set()
    for name in K.ORIGINAL:
        seen |= set(K.assignments(K.host_bytes(name)))
    assert seen == {0, 1, 8}
    assert 9 in K.assignments(K.host_bytes("small_plus_right")) and 10 in K.assignments(K.host_bytes("mid_side"))
    assert K.coded_number_bytes(K.host_bytes("blocks129")) == 2 and K.coded_number_bytes(K.host_bytes("blocks2049_mono")) == 3
    assert K.coded_number_bytes(K.host_bytes("sine_stereo")) == 1


# ---------------------------------------------------------------------------------------------------- the stand-alone program
def _case_file(path, name, sr=48000):
    pcm, data = K.pcm_of(name), K.host_bytes(name, sr)
    head = np.array([pcm.shape[1], sr, pcm.shape[0], len(data)], dtype="<i8")
    with open(path, "wb") as f:
        f.write(head.tobytes() + pcm.astype("<i2").tobytes() + data)


def _choices(line):
    d = dict(kv.split("=") for kv in line.split(": equal ")[1].split())
    return {k: (set() if v == "-" else {int(x) for x in v.split(",")}) if k in ("assign", "types", "orders", "porders") else int(v) for k, v in d.items()}


def test_frame_routines_under_host_sanitizers(tmp_path):
    """csrc/flac_out.h on the CPU, as the frame kernel calls it, lane after lane: every case's stream equals the host encoder's byte for
    byte, nothing draws a sanitizer report, and the choices the program prints cover every subframe kind, order, assignment and
    number length the encoder has."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "flac_out_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "flac_out_host.cpp"), "-o", str(exe)], check=True)
    cases = [(n, 48000) for n in K.ORIGINAL + K.ADDED + ("blocks129", "blocks2049_mono", "empty")] + [("rates", sr) for sr in K.RATES + (700001,)]
    files = []
    for name, sr in cases:
        files.append(str(tmp_path / f"{name}_{sr}.case"))
        _case_file(files[-1], name, sr)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) and all(": equal " in l for l in lines), r.stdout
    ch = {name if sr == 48000 else f"{name}_{sr}": _choices(l) for (name, sr), l in zip(cases, lines)}
    print(r.stdout)

    def union(names, key):
        return set().union(*[ch[n][key] for n in names])
    # the 13 original signals
    assert union(K.ORIGINAL, "assign") == {0, 1, 8} and union(K.ORIGINAL, "types") == {0, 1, 2} and union(K.ORIGINAL, "orders") == {0, 1, 2, 3, 4}
    assert union(K.ORIGINAL, "porders") == {0, 1, 3, 4} and max(ch[n]["kmax"] for n in K.ORIGINAL) <= 9
    # the five additions
    assert {9, 10} <= union(K.ADDED, "assign") and 8 in union(K.ADDED, "porders")
    assert max(ch[n]["kmax"] for n in K.ADDED) == 11
    assert max(ch[n]["run"] for n in K.ADDED) >= 750          # a unary run that spans 23 words
    assert ch["blocks129"]["numbytes"] == 2 and ch["blocks2049_mono"]["numbytes"] == 3 and ch["blocks2049_mono"]["frames"] == 2049
    assert ch["empty"]["frames"] == 0
