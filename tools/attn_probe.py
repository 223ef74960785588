#!/usr/bin/env python
"""Attention at the metric's shapes, and at one shape per remaining kernel instantiation, through the unit hook: error against fp32 torch
SDPA on the same bf16 inputs, and (under rocprofv3 --kernel-trace --stats) the kernel's own duration.  Env switches of attn.hip apply
(ACE355_ATTN_GQA, ACE355_ATTN_ROT, ...).  --reps N: launches per shape and run (default 8).  --libs A B A B ...: one run per named build of
libace355.so, in that order, shape by shape in ONE process on the same tensors (an A/B of two builds without the process-to-process
differences of separate runs; tools/attn_trace_medians.py reads the trace); default: one run of the tree's library."""
import ctypes as C, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ace355
from ace355 import native
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 8
native.lib()   # (torch's HIP runtime first; the plans below are this library's)
def load(path):   # a build of its own: own code object, own K rotation state
    h = C.CDLL(os.path.abspath(path))
    for name in ("ace355_attention", "ace355_gemm_set_k_rotation"):
        getattr(h, name).restype, getattr(h, name).argtypes = native.SIGNATURES[name]
    return h
LIBS = [(p, load(p)) for p in sys.argv[sys.argv.index("--libs") + 1:]] if "--libs" in sys.argv else [(native.LIB_PATH, native.lib())]
dev = torch.device("cuda:0"); P = native.ptr
# (N, Sq, Skv, Hq, Hkv, window), K rotation mode (None: the default).  The metric's four reach gqa<6> (three of them) and rot<3>; then one
# shape each for attn3<4>, attn3<8>, gqa<4> and, with the key-split kernel off under K rotation mode 0, gqa<3>.
SHAPES = [((16, 375, 375, 16, 8, -1), None), ((16, 375, 375, 16, 8, 128), None), ((8, 375, 769, 16, 8, -1), None), ((4, 1500, 1500, 16, 8, -1), None),
          ((2, 375, 375, 16, 8, -1), None), ((6, 1500, 1500, 16, 16, -1), None), ((12, 375, 375, 16, 8, 128), None), ((16, 100, 130, 16, 8, -1), 0)]
for (N, Sq, Skv, Hq, Hkv, win), krot in SHAPES:
    g = torch.Generator(device=dev).manual_seed(N + Sq + Skv)
    q = torch.randn(N, Sq, Hq * 128, device=dev, generator=g).to(torch.bfloat16); k = torch.randn(N, Skv, Hkv * 128, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(N, Skv, Hkv * 128, device=dev, generator=g).to(torch.bfloat16); o = torch.empty_like(q)
    prev = native.gemm_set_k_rotation(krot) if krot is not None else None
    p = native.attn_plan(N, Sq, Skv, Hq, Hkv, win, part_floats=native.ATTN_HOOK_PART_FLOATS)
    if prev is not None:
        native.gemm_set_k_rotation(prev)
    outs = []
    for _path, lib in LIBS:
        prev = lib.ace355_gemm_set_k_rotation(krot) if krot is not None else None
        for _ in range(REPS):
            native.check(lib.ace355_attention(P(q), P(k), P(v), P(o), N, Sq, Skv, Hq, Hkv, win, 128 ** -0.5, None))
        torch.cuda.synchronize()
        if prev is not None:
            lib.ace355_gemm_set_k_rotation(prev)
        outs.append(o.clone())
    qh = q.float().view(N, Sq, Hq, 128).transpose(1, 2); kh = k.float().view(N, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    vh = v.float().view(N, Skv, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, 1)
    sc = (qh @ kh.transpose(-1, -2)) * 128 ** -0.5
    if win >= 0:
        i = torch.arange(Sq, device=dev)[:, None]; j = torch.arange(Skv, device=dev)[None]
        sc = sc.masked_fill((i - j).abs() > win, float("-inf"))
    ref = (sc.softmax(-1) @ vh).transpose(1, 2).reshape(N, Sq, Hq * 128)
    print(f"N={N} Sq={Sq} Skv={Skv} Hq={Hq} Hkv={Hkv} win={win}{'' if krot is None else f' krot={krot}'} {p['kernel']}<{p['nw']}>: rel L2 vs fp32 "
          + " ".join(f"{float((x.float() - ref).norm() / ref.norm()):.3e}" for x in outs), flush=True)
