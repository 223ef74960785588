#!/usr/bin/env python
"""Record the encoder pass plans of 2 : 1 causal stacks (16 / 8 heads) as tests/golden/lm_plan_2to1.json.

The file in the repository was written by this script on the commit BEFORE the 4 : 1 head layout was added (run from that commit's
tree, whose library it imports), so tests/test_lm_gqa4_cpu.py can hold today's plans for two q heads per kv head to what they were
then, field for field.  Regenerating it on a later commit would make that test vacuous: do not.

Usage:  python tests/golden/make_lm_plan_2to1.py [output.json]
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (hidden, intermediate, heads, kv heads, layers, N, S, fields): the 0.6B and 1.7B LMs' widths in prefill, in decode steps on both
# sides of every boundary of the decode plan and in a text-encoder pass, and the small "wide" stack of the GPU tests.  Two layers each
# (a layer's steps differ from the next one's by the layer index alone) and one full 28-layer step, to keep the file small.
CACHE = dict(causal=1, has_cache=1, max_pos=4096, max_seqs=16, has_first=1)
REQUESTS = [(1024, 3072, 16, 8, 2, 2, 512, dict(CACHE, pos0=0)), (1024, 3072, 16, 8, 2, 16, 2048, dict(CACHE, pos0=0)),
            (2048, 6144, 16, 8, 2, 16, 300, dict(CACHE, pos0=0)), (1024, 3072, 16, 8, 2, 16, 256, dict(causal=1)),
            (512, 1024, 16, 8, 2, 3, 70, dict(CACHE, pos0=0, max_pos=1100, max_seqs=4)),
            (1024, 3072, 16, 8, 28, 16, 1, dict(CACHE, pos0=299))]
REQUESTS += [(D, F, 16, 8, 2, 16, 1, dict(CACHE, pos0=length - 1)) for D, F in ((1024, 3072), (2048, 6144))
             for length in (2, 64, 65, 256, 257, 1024, 1025, 4096)]


def evaluate():
    import ace355  # noqa: F401
    from ace355 import native
    return [{"request": list(r[:7]), "fields": r[7], "plan": native.encoder_pass_plan(*r[:7], **r[7])} for r in REQUESTS]


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lm_plan_2to1.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row, sort_keys=True) for row in evaluate()) + "\n]\n")
    print("wrote", path, os.path.getsize(path), "bytes")
