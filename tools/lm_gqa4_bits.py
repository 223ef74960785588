#!/usr/bin/env python
"""Are the 2 : 1 kernels' bits what they were before the 4 : 1 head layout?  -> profiles/lm_gqa4_bits.txt.

Two builds of the library - this tree's and one from the commit before the change (``--parent path/to/libace355.so``) - each loaded in
a child process of its own, run the same calls on the same weights:

* the LM: ``tests/_lm_oracle.py``'s WIDE stack (16 / 8 heads), a left-padded prefill of [3, 130] with first = (0, 5, 129) and 12
  teacher-forced decode steps (lengths 131 .. 142: three chunks of the decode cut) - fp32 logits of every step;
* the text encoder: ``tests/_textenc_oracle.py``'s TINY stack (4 / 2 heads), one pass over [3, 70] ids - bf16 hidden states.

Each child writes its outputs' raw bytes; the parent process compares them byte for byte and records a SHA-256 of each.  Exit status 1
when any differ.

Usage:  python tools/lm_gqa4_bits.py --parent /path/to/parent/libace355.so [--out profiles/lm_gqa4_bits.txt]
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P, STEPS = 130, 12


def child(lib_path: str, out_path: str) -> None:
    import numpy as np
    import torch   # first: the library resolves its HIP runtime to torch's (native.lib)

    import ace355  # noqa: F401
    from ace355 import native
    native.LIB_PATH = os.path.abspath(lib_path)
    have = ctypes.CDLL(native.LIB_PATH)
    native.SIGNATURES = {k: v for k, v in native.SIGNATURES.items() if hasattr(have, k)}   # an older build lacks the newer entries
    from ace355.lm import NativeCausalLM
    from ace355.textenc import NativeTextEncoder
    import _lm_oracle as L
    import _textenc_oracle as T

    dev = torch.device("cuda:0")
    out = {}
    lm = NativeCausalLM(L.WIDE, dev, max_positions=P + STEPS + 2, max_seqs=4)
    lm.load_state_dict(dict(L.weights("wide")))
    first = [0, 5, P - 1]
    ids, _ = L.left_padded([P - f for f in first], P, L.WIDE.vocab_size, 77)
    tail = torch.randint(0, L.WIDE.vocab_size, (3, STEPS), generator=torch.Generator().manual_seed(78))
    steps = [lm.prefill(ids, L.mask_of(first, P)).cpu()]
    for t in range(STEPS):
        steps.append(lm.decode(tail[:, t]).cpu())
    out["lm_logits"] = torch.stack(steps).numpy()
    lm.close()
    te = NativeTextEncoder(T.TINY, dev)
    te.load_state_dict(dict(T.weights(T.TINY, T.TINY_SEED)))
    tids = T.padded_ids((70, 33, 1), 70, T.TINY.vocab_size, 0, 79)
    hs = te(input_ids=tids).last_hidden_state
    out["textenc_hidden"] = hs.detach().cpu().contiguous().view(torch.int16).numpy()
    te.close()
    assert np.isfinite(out["lm_logits"]).all()
    np.savez(out_path, **out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libace355.so built from the commit before the change")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_gqa4_bits.txt"))
    ap.add_argument("--child", nargs=2, metavar=("LIB", "NPZ"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(*args.child)
        return 0
    if not args.parent or not os.path.exists(args.parent):
        ap.error("--parent: the library of the commit before the change")
    import numpy as np
    from ace355 import native
    libs = {"parent": os.path.abspath(args.parent), "this tree": native.LIB_PATH}
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (name, lib) in enumerate(libs.items()):
            npz = os.path.join(tmp, f"out{i}.npz")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, npz], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-4000:])
                return 2
            got[name] = dict(np.load(npz))
    lines = [f"# prefill [3, {P}] + {STEPS} decode steps of the WIDE LM (16 / 8 heads) and one TINY text-encoder pass (4 / 2 heads), on two builds",
             "# of the library, each in a child process of its own: raw bytes compared, SHA-256 of each recorded"]
    same = True
    for key in got["parent"]:
        a, b = got["parent"][key], got["this tree"][key]
        eq = a.shape == b.shape and a.tobytes() == b.tobytes()
        same &= eq
        lines.append(f"{key:<16} shape {tuple(a.shape)!s:<18} parent {hashlib.sha256(a.tobytes()).hexdigest()[:16]}  this tree "
                     f"{hashlib.sha256(b.tobytes()).hexdigest()[:16]}  {'bit-equal' if eq else 'DIFFERENT'}")
        if key == "lm_logits":
            for t in range(a.shape[0]):
                if a[t].tobytes() != b[t].tobytes():
                    lines.append(f"  step {t} ({'prefill' if t == 0 else 'decode'}) differs: max |a - b| = {float(np.abs(a[t] - b[t]).max()):.3e}")
    lines.append("result: " + ("every output bit-equal to the parent build's" if same else "outputs DIFFER from the parent build's"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
