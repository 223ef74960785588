#!/usr/bin/env python
"""One sha256 of the attention output per row of tests/_attn_plan_cases.py (ATTENTION_ROWS, ONE_ORDER_ROW, MASKED_ROWS, KEY_ROWS), each row
under its own K rotation mode and key lengths, after asserting that the plan is the row's (kernel, template argument, kv_split).  Two builds
of the library compute the same bits exactly when their listings are equal:

    python tools/attn_bits.py [--lib PATH]      (PATH: another build of libace355.so; default: the tree's)

Inputs are generator-seeded bf16 tensors made on the GPU, as tools/attn_probe.py makes them."""
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ace355  # noqa: E402, F401
from ace355 import native  # noqa: E402
import _attn_plan_cases as cases  # noqa: E402

if "--lib" in sys.argv:
    native.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])   # before the first native.lib()
lib = native.lib()
dev = torch.device("cuda:0")
P = native.ptr
print(f"# {native.LIB_PATH}")


def row_hash(shape, form, krot=None, lens=None):
    N, Sq, Skv, Hq, Hkv, win = shape
    prev = native.gemm_set_k_rotation(krot) if krot is not None else None
    try:
        p = native.attn_plan(*shape, part_floats=native.ATTN_HOOK_PART_FLOATS, **({"has_kv_len": 1} if lens is not None else {}))
        if form is not None:
            assert (p["kernel"], p["nw"], p["kv_split"]) == form, (shape, form, p)
        g = torch.Generator(device=dev).manual_seed(N + Sq + Skv)
        q = torch.randn(N, Sq, Hq * 128, device=dev, generator=g).to(torch.bfloat16)
        k = torch.randn(N, Skv, Hkv * 128, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(N, Skv, Hkv * 128, device=dev, generator=g).to(torch.bfloat16)
        o = torch.zeros_like(q)
        if lens is None:
            native.check(lib.ace355_attention(P(q), P(k), P(v), P(o), N, Sq, Skv, Hq, Hkv, win, 128 ** -0.5, None), "attention")
        else:
            native.check(lib.ace355_attention_masked(P(q), P(k), P(v), P(o), N, Sq, Skv, Hq, Hkv, win, 128 ** -0.5, (C.c_int32 * N)(*lens), None),
                         "attention_masked")
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            native.gemm_set_k_rotation(prev)
    digest = hashlib.sha256(o.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    tag = f"{p['kernel']}<{p['nw']}>" + (f" split {p['kv_split']}" if p["kv_split"] > 1 else "")
    opts = (f" krot {krot}" if krot is not None else "") + (f" lens {tuple(lens)}" if lens is not None else "")
    print(f"{str(shape):34s} {tag:16s}{opts}: {digest}", flush=True)


print("## ATTENTION_ROWS")
for shape, form in cases.ATTENTION_ROWS:
    row_hash(shape, form)
print("## ONE_ORDER_ROW")
row_hash(*cases.ONE_ORDER_ROW, krot=0)
print("## MASKED_ROWS (the lengths of tests/test_cond_gpu.py::test_attention_key_padding_mask; the rows name no form)")
for shape, lens in zip(cases.MASKED_ROWS, ([300, 90, 1], [37, 0], [129, 64])):
    row_hash(shape, None, lens=lens)
print("## KEY_ROWS")
for shape, form, opts in cases.KEY_ROWS:
    row_hash(shape, form, krot=opts.get("krot"), lens=opts.get("lens"))
