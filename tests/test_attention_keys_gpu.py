"""GPU: every softmax weight of every attention kernel form, read back through a one-hot V (tests/_attn_keys.py) and held, element by
element, to the fp64 softmax over the keys the DEFINITION makes visible: an invisible key weighs exactly 0, a visible one is within
(2 U + U^2 + 2^-12) p of its weight and above 0.  A relative L2 over the output (tests/test_kernels_gpu.py::test_attention) cannot see one
band-edge key, one leaked pad key or an empty split-KV part; this can.  The rows, each with the launch form it was chosen for, are
_attn_plan_cases.KEY_ROWS; tests/test_attn_plan_cpu.py checks what they reach together, tests/test_attn_keys_cpu.py that the method
discriminates.

Largest |got - p| / p measured on an MI355X, per form over its rows (masked rows included), in units of U = 2^-8; the bound is 2.0664 U:

    attn3<4> 1.884    attn3<4> split-KV + merge 1.943    attn3<8> 1.956    gqa<3> 1.948    gqa<4> 1.970    gqa<6> 1.969    rot<3> 1.948

With attn3_kernel's band predicate changed from `<=` to `<` (a scratch build) every window-128 row of test_attention still passes and
the (1, 300, 300, 3, 1, 128) row here fails on 19508 elements."""
import ctypes as C

import pytest
import torch

import _attn_keys as keys
import _attn_plan_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", cases.KEY_ROWS, ids=[cases.key_row_id(r) for r in cases.KEY_ROWS])
def test_attention_weights(gpu_device, row):
    from ace355 import native
    lib = native.lib()
    shape, form, opts = row
    N, Sq, Skv, Hq, Hkv, window = shape
    lens = opts.get("lens")
    if lens is not None:
        assert len(lens) == N and Skv in lens and 0 in lens and any(x % 64 for x in lens)
    kv = None if lens is None else (C.c_int32 * N)(*lens)

    def attend(q, k, v):
        out = torch.full((N, Sq, Hq * 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)   # a row left unwritten fails
        if lens is None:
            rc = lib.ace355_attention(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(out), N, Sq, Skv, Hq, Hkv, window, keys.SCALE, None)
        else:
            rc = lib.ace355_attention_masked(native.ptr(q), native.ptr(k), native.ptr(v), native.ptr(out), N, Sq, Skv, Hq, Hkv, window,
                                             keys.SCALE, kv, None)
        native.check(rc, "attention")
        torch.cuda.synchronize()
        return out

    prev = native.gemm_set_k_rotation(opts["krot"]) if "krot" in opts else None
    try:
        p = native.attn_plan(N, Sq, Skv, Hq, Hkv, window, part_floats=native.ATTN_HOOK_PART_FLOATS, **({"has_kv_len": 1} if lens is not None else {}))
        assert (p["kernel"], p["nw"], p["kv_split"]) == form, p
        res = keys.run_case(shape, lens, attend, seed=Sq + Skv + Hq, pairs=opts.get("pairs"), device=gpu_device, label=cases.key_row_id(row))
    finally:
        if prev is not None:
            native.gemm_set_k_rotation(prev)
    print(f"{cases.key_row_id(row)}: {form[0]}<{form[1]}> x {form[2]} part(s), {res['runs']} runs, max |got - p| / p = {res['max_err_u']:.3f} U, "
          f"smallest visible p {res['min_p']:.3g}")
    assert res["min_p"] > keys.P_FLOOR      # "a visible key weighs more than 0" is an honest demand of bf16 / fp32
    assert res["n_bad"] == 0, res["report"]
