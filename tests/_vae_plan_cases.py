"""The conv requests and VAE calls whose plans tests/vae_plan_table.json records, the launch forms the GPU tests claim for their cases,
and the evaluator behind tests/test_vae_plan_cpu.py.

    python tests/_vae_plan_cases.py --write     regenerate the table (after a deliberate change of csrc/vae_plan.h)
    python tests/_vae_plan_cases.py --properties   check the data-flow properties of the step lists under THIS process's switches
    python tests/_vae_plan_cases.py --plans     print the table rows' plans of THIS process (its ACE355_CONV_* / ACE355_VAE_* environment) as JSON

A conv request is a dict of ace355_conv_request fields (include/ace355.h), a VAE call is (configuration keywords, encoder?, items,
latent frames).  No GPU is needed: ace355_conv_plan / ace355_vae_plan evaluate the library's pure plan_conv / plan_vae.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "vae_plan_table.json")

SMALL = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
FULL = dict()
ONE_BLOCK = dict(decoder_channels=128, channel_multiples=(2,), downsampling_ratios=(4,))
ODD_HOP = dict(decoder_channels=64, channel_multiples=(1, 2, 3), downsampling_ratios=(3, 5, 7))
CONFIGS = {"small": SMALL, "full": FULL, "one-block": ONE_BLOCK, "odd-hop": ODD_HOP}

# conv_kernel<bn, tm, ws> by the names the tests use
FORMS = {(32, 128, 0): "n32",    # 32-column tile, 4 waves (N < 128)
         (128, 128, 0): "w4",    # 128 x 128 tile, 4 waves
         (128, 256, 0): "w8",    # 256 x 128 tile, 8 waves
         (128, 256, 1): "f8"}    # the one-launch residual unit on 8 waves of 32 rows x 128 channels


def form(plan):
    return FORMS[(plan["bn"], plan["tm"], plan["ws"])]


# tests/test_vae_layers_gpu.py's cases: (id, configuration, encoder?, items, latent frames, the form every launch takes unless
# {(weight, Cin): form} says otherwise).  The GPU tests assert these against native.vae_plan before they launch.
LAYER_CASES = [
    # widths 256 / 128 / 64, odd lengths 37, 222, 888, 1776: the C = 64 units and the output conv on the 32-column tile, the C = 128
    # units as one launch on 4 waves, everything else 4-wave (largest wgs128 = 14 * 1 * 2)
    ("small-B2-T37", SMALL, False, 2, 37, "w4", {("unit_c1", 64): "n32", ("unit_c2", 64): "n32", ("out", 64): "n32"}),
    # every 4-wave form of the full widths (largest wgs128: block 0's transposed conv, 80; one-launch units at C = 128: 180 and 360 < 1400)
    ("full-B1-T24", FULL, False, 1, 24, "w4", {("out", 128): "n32"}),
    # every decoder launch on the form of the 8 x 30 s run: transposed convs (plain rows, wgs128 >= 1500) and k = 7 convs (>= 1400; block
    # 0's sits at 22 * 8 * 8 = 1408, T = 268 would give 1344) on 8 waves, the one-launch units on the 8-wave form; conv1 (Cin = 64) and
    # the k = 1 convs (residual) 4-wave by design
    ("full-B8-T280", FULL, False, 8, 280, "w4", {("out", 128): "n32", ("unit_c1", 128): "f8", **{("convt", c): "w8" for c in (2048, 1024, 512, 256, 128)},
                                                  **{("unit_c1", c): "w8" for c in (1024, 512, 256)}}),
    ("small-B2-23", SMALL, True, 2, 23, "w4", {}),
    # L = 23040: one-launch units at C = 128 on 4 waves (180 * 2 = 360), the strided convs over the shifted view never tall
    ("full-B2-12", FULL, True, 2, 12, "w4", {}),
    # L = 360960: k = 7 at C = 256 (353 * 2 * 4 = 2824) and C = 512 (89 * 4 * 4 = 1424) on 8 waves, the one-launch units on the 8-wave
    # form (2820 * 4, 1410 * 4); C = 1024 (15 * 8 * 4 = 480) stays 4-wave
    ("full-B4-188", FULL, True, 4, 188, "w4", {("unit_c1", 128): "f8", ("unit_c1", 256): "w8", ("unit_c1", 512): "w8"}),
]
# tests/test_vae_gpu.py::test_fused_unit_forms_agree_bit_for_bit: its decode and its encode run the one-launch units on 4 waves by
# default (ACE355_CONV_F8=0 the same) and on the 8-wave form under ACE355_CONV_F8=1
FUSED_FORM_CALLS = [(FULL, False, 2, 41), (FULL, True, 1, 12)]
# tests/test_vae_gpu.py::test_decode_vs_oracle
ORACLE_CALLS = [(SMALL, False, 2, 37), (FULL, False, 1, 24), (FULL, False, 2, 9)]

# tests/test_kernels_gpu.py::test_conv1d_nlc's rows (B, L, Cin, Cout, taps, dil, snake, res), each with the form it was chosen for
CONV1D_ROWS = [
    ((2, 300, 128, 128, 7, 1, True, False), "w4"), ((1, 517, 128, 128, 7, 9, True, False), "w4"), ((2, 200, 256, 256, 7, 3, True, False), "w4"),
    ((2, 300, 128, 128, 1, 1, True, True), "w4"), ((1, 40, 64, 2048, 7, 1, False, False), "w4"), ((1, 1000, 128, 2, 7, 1, True, False), "n32"),
    # wgs128 = 516 * 2 * 4 = 4128, but a residual keeps a launch off the 8-wave form; and its residual-free twin on it
    ((4, 66000, 256, 256, 7, 3, True, True), "w4"), ((4, 66000, 256, 256, 7, 3, True, False), "w8"),
    # wgs128 = 235 * 4 * 8 = 7520: 8 waves, dilation 9, with and without the Snake
    ((8, 30000, 512, 512, 7, 9, True, False), "w8"), ((8, 30000, 512, 512, 7, 9, False, False), "w8"),
]
ALL_FORMS = set(FORMS.values())


def conv1d_request(row):
    B, L, Cin, Cout, taps, _dil, snake, res = row
    return dict(B=B, M=L, N=Cout, Cin=Cin, taps=taps, in_snake=int(snake), x_view=0, res=int(res), fused=0)


def vae_config(kw):
    import ace355
    return ace355.VaeConfig(**kw)


def vae_call(kw, enc, B, frames, **budget):
    """native.vae_plan of a call given in latent frames (an encode takes hop * frames samples)."""
    from ace355 import native
    cfg = vae_config(kw)
    return native.vae_plan(cfg, enc, B, frames * cfg.hop if enc else frames, **budget)


def step_request(plan, st):
    return dict(B=plan["items_per_window"], M=st["M"], N=st["N"], Cin=st["Cin"], taps=st["taps"], in_snake=int(st["in_snake"] is not None),
                x_view=int(st["x_valid"] != 0), res=int(st["res"] is not None), fused=st["fused"])


def step_name(st):
    return st["weight"] + (f" b{st['block']}" if st["block"] >= 0 else "") + (f" u{st['unit']}" if st["unit"] >= 0 else "")


def assert_forms(plan, default, special, tag=""):
    """Every step of a native.vae_plan result is on the form its case claims."""
    for st in plan["steps"]:
        want = special.get((st["weight"], st["Cin"]), default)
        assert form(st["plan"]) == want, f"{tag}: {step_name(st)} Cin={st['Cin']} M={st['M']} is planned on {form(st['plan'])}, the case says {want}"


def calls():
    """(name, configuration, encoder?, items, frames): every VAE call whose conv launches the table pins."""
    out = [(f"decode {n} x T=750", FULL, False, n, 750) for n in (1, 2, 4, 8)]   # (8 x 30 s is the bench's decode)
    out += [("decode 1 x T=3000", FULL, False, 1, 3000), ("encode 1 x 30 s", FULL, True, 1, 750), ("encode 4 x 30 s", FULL, True, 4, 750)]
    out += [(f"test_vae_layers {cid}", kw, enc, B, fr) for cid, kw, enc, B, fr, _d, _s in LAYER_CASES]
    out += [(f"test_decode_vs_oracle {'small' if kw else 'full'} B={B} T={T}", kw, enc, B, T) for kw, enc, B, T in ORACLE_CALLS]
    return out


def conv_rows():
    """(name, request): the distinct conv requests of every call, in launch order, then test_conv1d_nlc's."""
    rows, seen = [], set()
    for name, kw, enc, B, fr in calls():
        plan = vae_call(kw, enc, B, fr)
        for i, st in enumerate(plan["steps"]):
            rq = step_request(plan, st)
            key = tuple(sorted(rq.items()))
            if key not in seen:   # (the three units of a block, a call repeated by another test)
                seen.add(key)
                rows.append((f"{name}: step {i} {step_name(st)}", rq))
    rows += [(f"test_conv1d_nlc: {r}", conv1d_request(r)) for r, _f in CONV1D_ROWS]
    return rows


# the four full step lists the table pins (defaults)
VAE_ROWS = [("small decode B=2 T=37", SMALL, False, 2, 37), ("small encode B=2 23 frames", SMALL, True, 2, 23),
            ("full decode B=1 T=24", FULL, False, 1, 24), ("full encode B=2 12 frames", FULL, True, 2, 12)]


def evaluate(rows=None):
    """The table of this process.  ``rows``: the conv requests to plan (a child process under a switch plans the TABLE's requests: the
    switch may change which requests a call makes, and that shows in the step lists)."""
    from ace355 import native
    return {"conv": [{"name": n, "request": r, "plan": native.conv_plan(**r)} for n, r in (rows or conv_rows())],
            "vae": [{"name": n, "plan": vae_call(kw, enc, B, fr)} for n, kw, enc, B, fr in VAE_ROWS]}


# ---------------------------------------------------------------------------------------------- what a step list must satisfy
# The public stage lists of the four VAE_ROWS as the library produced them BEFORE the list was read off the plan (the hand-written
# stage_list of csrc/vae.hip), under the default switches: (kind, block, unit, channels, flags, src, res, dilation, rows).
STAGE_FIELDS = ("kind", "block", "unit", "channels", "flags", "src", "res", "dilation", "rows")
EXPECTED_STAGES = {
    "small decode B=2 T=37": [
        (0,-1,-1,64,0,-1,-1,1,37), (1,-1,-1,256,2,0,-1,1,37), (2,0,-1,128,0,1,-1,1,222), (3,0,0,128,5,2,2,1,222), (3,0,1,128,5,3,3,3,222),
        (3,0,2,128,7,4,4,9,222), (2,1,-1,64,0,5,-1,1,888), (4,1,0,64,3,6,-1,1,888), (5,1,0,64,0,7,6,1,888), (4,1,1,64,3,8,-1,3,888),
        (5,1,1,64,0,9,8,1,888), (4,1,2,64,3,10,-1,9,888), (5,1,2,64,2,11,10,1,888), (2,2,-1,64,0,12,-1,1,1776), (4,2,0,64,3,13,-1,1,1776),
        (5,2,0,64,0,14,13,1,1776), (4,2,1,64,3,15,-1,3,1776), (5,2,1,64,0,16,15,1,1776), (4,2,2,64,3,17,-1,9,1776),
        (5,2,2,64,2,18,17,1,1776),
    ],
    "small encode B=2 23 frames": [
        (0,-1,-1,64,0,-1,-1,1,1104), (1,-1,-1,128,0,0,-1,1,1104), (3,0,0,128,5,1,1,1,1104), (3,0,1,128,5,2,2,3,1104),
        (3,0,2,128,7,3,3,9,1104), (6,0,-1,128,0,4,-1,1,552), (3,1,0,128,5,5,5,1,552), (3,1,1,128,5,6,6,3,552), (3,1,2,128,7,7,7,9,552),
        (6,1,-1,256,0,8,-1,1,138), (4,2,0,256,3,9,-1,1,138), (5,2,0,256,0,10,9,1,138), (4,2,1,256,3,11,-1,3,138),
        (5,2,1,256,0,12,11,1,138), (4,2,2,256,3,13,-1,9,138), (5,2,2,256,2,14,13,1,138), (6,2,-1,512,2,15,-1,1,23),
        (7,-1,-1,128,8,16,-1,1,23),
    ],
    "full decode B=1 T=24": [
        (0,-1,-1,64,0,-1,-1,1,24), (1,-1,-1,2048,2,0,-1,1,24), (2,0,-1,1024,0,1,-1,1,240), (4,0,0,1024,3,2,-1,1,240),
        (5,0,0,1024,0,3,2,1,240), (4,0,1,1024,3,4,-1,3,240), (5,0,1,1024,0,5,4,1,240), (4,0,2,1024,3,6,-1,9,240), (5,0,2,1024,2,7,6,1,240),
        (2,1,-1,512,0,8,-1,1,1440), (4,1,0,512,3,9,-1,1,1440), (5,1,0,512,0,10,9,1,1440), (4,1,1,512,3,11,-1,3,1440),
        (5,1,1,512,0,12,11,1,1440), (4,1,2,512,3,13,-1,9,1440), (5,1,2,512,2,14,13,1,1440), (2,2,-1,256,0,15,-1,1,5760),
        (4,2,0,256,3,16,-1,1,5760), (5,2,0,256,0,17,16,1,5760), (4,2,1,256,3,18,-1,3,5760), (5,2,1,256,0,19,18,1,5760),
        (4,2,2,256,3,20,-1,9,5760), (5,2,2,256,2,21,20,1,5760), (2,3,-1,128,0,22,-1,1,23040), (3,3,0,128,5,23,23,1,23040),
        (3,3,1,128,5,24,24,3,23040), (3,3,2,128,7,25,25,9,23040), (2,4,-1,128,0,26,-1,1,46080), (3,4,0,128,5,27,27,1,46080),
        (3,4,1,128,5,28,28,3,46080), (3,4,2,128,7,29,29,9,46080),
    ],
    "full encode B=2 12 frames": [
        (0,-1,-1,64,0,-1,-1,1,23040), (1,-1,-1,128,0,0,-1,1,23040), (3,0,0,128,5,1,1,1,23040), (3,0,1,128,5,2,2,3,23040),
        (3,0,2,128,7,3,3,9,23040), (6,0,-1,128,0,4,-1,1,11520), (3,1,0,128,5,5,5,1,11520), (3,1,1,128,5,6,6,3,11520),
        (3,1,2,128,7,7,7,9,11520), (6,1,-1,256,0,8,-1,1,2880), (4,2,0,256,3,9,-1,1,2880), (5,2,0,256,0,10,9,1,2880),
        (4,2,1,256,3,11,-1,3,2880), (5,2,1,256,0,12,11,1,2880), (4,2,2,256,3,13,-1,9,2880), (5,2,2,256,2,14,13,1,2880),
        (6,2,-1,512,0,15,-1,1,720), (4,3,0,512,3,16,-1,1,720), (5,3,0,512,0,17,16,1,720), (4,3,1,512,3,18,-1,3,720),
        (5,3,1,512,0,19,18,1,720), (4,3,2,512,3,20,-1,9,720), (5,3,2,512,2,21,20,1,720), (6,3,-1,1024,0,22,-1,1,120),
        (4,4,0,1024,3,23,-1,1,120), (5,4,0,1024,0,24,23,1,120), (4,4,1,1024,3,25,-1,3,120), (5,4,1,1024,0,26,25,1,120),
        (4,4,2,1024,3,27,-1,9,120), (5,4,2,1024,2,28,27,1,120), (6,4,-1,2048,2,29,-1,1,12), (7,-1,-1,128,8,30,-1,1,12),
    ],
}


def stages_of(plan, enc, zc=64):
    """The public stage list of a native.vae_plan result: the input image, then every step that stores a stage."""
    out = [(0, -1, -1, 64 if enc else zc, 0, -1, -1, 1, plan["window_len"])]
    for st in plan["steps"]:
        if st["stage"] >= 0:
            assert st["stage"] == len(out), "stages are numbered in launch order"
            out.append(tuple(st["stage_info"][f] for f in STAGE_FIELDS))
    assert len(out) == plan["n_stages"]
    return out


def check_properties(plan, tag=""):
    """Data flow of a step list: every source was written (or is the input image), nothing is read after it was overwritten, a fused
    unit writes to the slot it does not read, an activation that carries its reader's Snake has exactly one reader and that reader
    applies no Snake, the buffer size covers every step, and each step's conv plan is its request's."""
    from ace355 import native
    steps = plan["steps"]
    writer = {"in": -1}   # buffer -> index of the step whose result it holds
    readers = {}          # step index -> indices of the steps that read its result
    for i, st in enumerate(steps):
        for role in ("src", "res"):
            b = st[role]
            if b is None:
                continue
            assert b in writer, f"{tag} step {i}: reads {b} before anything wrote it"
            readers.setdefault(writer[b], []).append((i, role))
        if st["fused"]:
            assert st["dst"] != st["src"] and st["res"] == st["src"], f"{tag} step {i}: a fused unit writes to the slot it does not read"
        elif st["res"] is not None:
            assert st["dst"] == st["res"] != st["src"], f"{tag} step {i}: the k = 1 conv adds the unit's input in place"
        else:
            assert st["dst"] != st["src"], f"{tag} step {i}: in place without a residual"
        if st["dst"].startswith("slot"):
            assert st["y_valid"] <= plan["slot_elems"] and st["out_mode"] == 0, f"{tag} step {i}: larger than the buffers"
        writer[st["dst"]] = i
        assert st["plan"] == native.conv_plan(**step_request(plan, st)), f"{tag} step {i}: not plan_conv of its request"
    # (a read "after a later step overwrote it" would show as a reader attributed to the wrong writer: check by replay that every
    #  step reads the result of the launch its stage_info names)
    stage_step = {st["stage"]: i for i, st in enumerate(steps) if st["stage"] >= 0}
    for w, rs in readers.items():
        for i, role in rs:
            si = steps[i]["stage_info"]
            if si is not None:
                want = si["src" if role == "src" else "res"]
                assert (w == -1 and want == 0) or stage_step.get(want) == w, f"{tag} step {i}: reads another stage than it names"
    for i, st in enumerate(steps):
        if st["out_snake"] is not None:
            rs = readers.get(i, [])
            assert len(rs) == 1 and rs[0][1] == "src" and steps[rs[0][0]]["in_snake"] is None, f"{tag} step {i}: OUT_SNAKE needs one reader without IN_SNAKE"
    assert steps[-1]["dst"] == "out" and all(st["dst"] != "out" for st in steps[:-1]) and all(st["dst"] != "in" for st in steps)


PROPERTY_LENGTHS = (1, 2, 7, 23, 37, 100)   # latent frames; the encoder also takes hop * frames + a ragged remainder


def run_properties():
    """Every configuration, both halves, PROPERTY_LENGTHS, under this process's switches.  Returns the number of plans checked."""
    from ace355 import native
    n = 0
    for cname, kw in CONFIGS.items():
        cfg = vae_config(kw)
        for frames in PROPERTY_LENGTHS:
            for B in (1, 3):
                p = native.vae_plan(cfg, False, B, frames)
                check_properties(p, f"{cname} decode B={B} T={frames}")
                # (an odd stride's transposed conv gives s L - 1 samples: k = 2 s, pad = ceil(s / 2))
                assert p["window_len"] == frames and (p["out_len"] == cfg.hop * frames or any(r % 2 for r in cfg.downsampling_ratios))
                for extra in (0, cfg.hop // 2 + 1):
                    p = native.vae_plan(cfg, True, B, cfg.hop * frames + extra)
                    check_properties(p, f"{cname} encode B={B} L={cfg.hop * frames + extra}")
                    if not extra:
                        assert p["out_len"] == frames, "latent_frames(hop * n) = n"
                    n += 1
                n += 1
    return n


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ace355  # noqa: F401
    if "--write" in sys.argv:
        t = evaluate()
        with open(TABLE, "w") as f:
            f.write('{"conv": [\n' + ",\n".join(json.dumps(r) for r in t["conv"]) + '\n],\n"vae": [\n' + ",\n".join(json.dumps(r) for r in t["vae"]) + "\n]}\n")
        print("wrote", TABLE)
    elif "--properties" in sys.argv:
        print(json.dumps({"checked": run_properties()}))
    elif "--plans" in sys.argv:
        print(json.dumps(evaluate([(r["name"], r["request"]) for r in json.load(open(TABLE))["conv"]])))
