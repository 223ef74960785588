"""GPU: teacher-forced LM scoring (csrc/lm_score.hip, ``NativeCausalLM.score``, ``ace355.lmscore``): per target token one log-probability
and one 0-based rank, with no logits stored.

1. the rows kernel against fp64 on the same bf16 inputs; 2. the handle path against the oracle (tests/_lm_oracle.py) under the project's
rule (tests/_drift.py); 3. what a score leaves of the handle; 4. refusals before any launch; 5. the seam on fixture G24's request.
"""
import ctypes as C

import pytest
import torch

import _drift
import _lm_oracle as L
import _lm_score_ref as S

pytestmark = pytest.mark.gpu

CHUNK = 1024   # ids per workgroup (csrc/lm_plan.h); test_rows_plan_is_what_the_cases_assume pins it
MAX_POS = 128


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _record(line):
    """A measured figure (profiles/lm_score_parity.txt keeps these lines of one run)."""
    print("    " + line)


# ------------------------------------------------------------------------------------------------ 1. the rows kernel
# (R, V, D, x row stride or None, use a row_index list)
ROWS_CASES = [(1, 1003, 256, None, False), (17, 1003, 256, None, False), (70, 2051, 512, 528, True), (70, 8193, 2048, None, False),
              (33, CHUNK + 1, 256, None, False)]
_ROWS = {}


def _rows_case(R, V, D):
    """bf16 x [R, D], W [V, D] (logit std about 1) and targets: row r aims at fp64 rank r mod 13; row 0 is the argmax; with R >= 17 row 1
    targets id 0, row 2 id V - 1, rows 3 and 4 share one id, and row 5 targets id 7 of three IDENTICAL W rows 5, 7, 9 (a tie: id 5 is
    ahead of it, id 9 behind).  The fp64 and fp32 host references are computed once and shared."""
    key = (R, V, D)
    if key not in _ROWS:
        g = torch.Generator().manual_seed(R * 1000003 + V * 101 + D)
        x = torch.randn(R, D, generator=g).to(torch.bfloat16)
        W = (torch.randn(V, D, generator=g) / D ** 0.5).to(torch.bfloat16)
        if R >= 17:
            W[5] = W[7]
            W[9] = W[7]
        l64 = x.double() @ W.double().T
        l32 = x.float() @ W.float().T
        order = torch.sort(l64, dim=1, descending=True, stable=True).indices
        t = torch.stack([order[r, r % 13] for r in range(R)])
        if R >= 17:
            t[1], t[2], t[3], t[5] = 0, V - 1, t[4], 7
        lp64, rank64 = S.token_stats(l64, t)
        lp32, _ = S.token_stats(l32, t)
        rows = torch.arange(R)
        m32 = float((l32.double() - l64).abs().max())
        dist = (l64 - l64[rows, t][:, None]).abs()
        dist[rows, t] = float("inf")
        _ROWS[key] = dict(x=x, W=W, t=t.to(torch.int32), lp64=lp64, lp32=lp32, rank64=rank64, m32=m32, gap=dist.min(1).values,
                          near=(dist <= 8.0 * m32).sum(1))
    return _ROWS[key]


def _place(c, stride, indexed, dev):
    """x on the device as the case asks: dense, or rows scattered (reversed, every other row) in a wider, longer buffer."""
    x = c["x"]
    R, D = x.shape
    if stride is None and not indexed:
        return x.to(dev), None
    buf = torch.full((2 * R + 3, stride or D), 7.0, dtype=torch.bfloat16)
    idx = torch.tensor([2 * (R - 1 - r) + 1 for r in range(R)], dtype=torch.int32)
    buf[idx.long(), :D] = x
    return buf.to(dev)[:, :D], idx.to(dev)


@pytest.mark.parametrize("R,V,D,stride,indexed", ROWS_CASES)
def test_rows_against_fp64(gpu_device, R, V, D, stride, indexed):
    """Log-prob: |d| <= max(2 x the fp32 host computation's distance from fp64 on these inputs, 4 ulp of the fp32 result).  Rank: exact
    on every row whose fp64 gap to the nearest other logit exceeds 8 x m32 (m32 = the fp32 HOST logits' largest error: two independent
    fp32 summation orders, with headroom); elsewhere off by at most the number of fp64 logits that close; at most 10 % such rows."""
    from ace355 import lmscore
    c = _rows_case(R, V, D)
    xd, idx = _place(c, stride, indexed, gpu_device)
    Wd, td = c["W"].to(gpu_device), c["t"].to(gpu_device)
    lp, rank = lmscore.score_rows(xd, Wd, td, idx)
    lp2, rank2 = lmscore.score_rows(xd, Wd, td, idx)
    assert lp.shape == (R,) and lp.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(rank, rank2), "two calls differ"
    lp, rank = lp.cpu(), rank.cpu()
    assert torch.isfinite(lp).all() and bool((lp <= 0).all())

    d32 = float((c["lp32"].double() - c["lp64"]).abs().max())
    err = (lp.double() - c["lp64"]).abs()
    a32 = c["lp32"].abs()
    ulp4 = 4.0 * (torch.nextafter(a32, torch.full_like(a32, float("inf"))) - a32).double()
    gate = torch.maximum(torch.full_like(ulp4, 2.0 * d32), ulp4)
    _record(f"rows ({R},{V},{D}): log-prob max|gpu - fp64| {float(err.max()):.3e}, fp32 host {d32:.3e}, ratio "
            f"{float(err.max()) / max(d32, 1e-300):.2f}, worst err / gate {float((err / gate).max()):.2f}, m32 {c['m32']:.2e}, "
            f"median gap {float(c['gap'].median()):.2e}")
    assert bool((err <= gate).all()), (err / gate).tolist()

    decided = c["gap"] > 8.0 * c["m32"]
    drank = (rank.long() - c["rank64"].long()).abs()
    assert int((~decided).sum()) * 10 <= R, f"{int((~decided).sum())} of {R} rows undecided"
    assert torch.equal(rank[decided], c["rank64"][decided]), (rank.tolist(), c["rank64"].tolist())
    assert bool((drank <= c["near"]).all()), (drank.tolist(), c["near"].tolist())
    if R >= 17:
        # identical W rows give identical logits: ordered by id, and exactly so, because the threshold is the head's own arithmetic
        assert int(rank[5]) == int(c["rank64"][5]), (int(rank[5]), int(c["rank64"][5]))
        assert int(rank[0]) == 0


@pytest.mark.parametrize("R,V,D", [(70, 2051, 512), (70, 8193, 2048)])
def test_a_row_alone_has_the_bits_it_has_in_the_batch(gpu_device, R, V, D):
    from ace355 import lmscore
    c = _rows_case(R, V, D)
    xd, Wd, td = c["x"].to(gpu_device), c["W"].to(gpu_device), c["t"].to(gpu_device)
    lp, rank = lmscore.score_rows(xd, Wd, td)
    for r in (0, 37, 64, 69):
        lp1, rank1 = lmscore.score_rows(xd[r:r + 1], Wd, td[r:r + 1].contiguous())
        assert torch.equal(_bits(lp1), _bits(lp[r:r + 1])) and int(rank1[0]) == int(rank[r]), r


def test_rows_plan_is_what_the_cases_assume():
    from ace355 import native
    p = native.lm_score_plan(33, CHUNK + 1, 256)
    assert p["chunk"] == CHUNK and p["chunks"] == 2 and p["tile_rows"] == 64 and (p["grid_x"], p["grid_y"]) == (1, 2)
    assert native.lm_score_plan(70, 8193, 2048)["grid_x"] == 2


def test_rows_refusals(gpu_device):
    """Before any launch: a workspace that is too small, sizes outside the limits, a misaligned stride, null pointers."""
    from ace355 import native
    lib = native.lib()
    R, V, D = 4, 1003, 256
    x = torch.zeros(R, D, dtype=torch.bfloat16, device=gpu_device)
    W = torch.zeros(V, D, dtype=torch.bfloat16, device=gpu_device)
    t = torch.zeros(R, dtype=torch.int32, device=gpu_device)
    lp = torch.full((R,), 3.0, device=gpu_device)
    rank = torch.full((R,), -7, dtype=torch.int32, device=gpu_device)
    need = native.lm_score_workspace_bytes(R, V)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)

    def call(R_=R, V_=V, D_=D, stride=D, ws_bytes=need, x_=x, t_=t):
        return lib.ace355_lm_score_rows(native.ptr(x_), stride, None, native.ptr(W), native.ptr(t_), R_, V_, D_, native.ptr(lp),
                                        native.ptr(rank), native.ptr(ws), ws_bytes, native.current_stream_ptr())

    assert need > 0 and native.lm_score_workspace_bytes(0, V) == 0 and native.lm_score_workspace_bytes(R, 0) == 0
    assert call(ws_bytes=need - 1) == 1 and "workspace of" in native.last_error()
    assert call(R_=0) == 1 and call(R_=native.LM_MAX_TOKENS + 1) == 1
    assert call(V_=0) == 1 and call(V_=(1 << 20) + 1) == 1
    assert call(D_=96) == 1 and "multiple of 64" in native.last_error()
    assert call(stride=D - 8) == 1 and call(stride=D + 4) == 1
    assert call(x_=None) == 1 and call(t_=None) == 1
    torch.cuda.synchronize()
    assert bool((lp == 3.0).all()) and bool((rank == -7).all()), "a refused call wrote its outputs"
    assert call() == 0


# ------------------------------------------------------------------------------------------------ 2. - 4. the handle
@pytest.fixture(scope="module")
def lms(gpu_device):
    from ace355.lm import NativeCausalLM
    made = {}

    def get(name, fresh=False):
        if fresh or name not in made:
            lm = NativeCausalLM(L.CONFIGS[name], gpu_device, max_positions=MAX_POS, max_seqs=4)
            lm.load_state_dict(dict(L.weights(name)))
            if fresh:
                made[f"{name}#{len(made)}"] = lm
                return lm
            made[name] = lm
        return made[name]

    yield get
    for lm in made.values():
        lm.close()


def _oracle_stats(name, ids, first, start):
    """Per scored token, from one causal pass of the fp32 oracle and one of its bf16-storage emulation: the oracle's log-prob and
    rank, the emulation's log-prob, and the number of oracle logits within twice the emulation's largest logit error of the target's."""
    cfg, w = L.CONFIGS[name], L.weights(name)
    N, P = ids.shape
    with torch.no_grad():
        ref = L.lm_logits_at(cfg, w, ids, first, range(P))
        emu = _drift.emulated(L.lm_logits_at, cfg, w, ids, first, range(P))
    rows = [(n, c) for n in range(N) for c in range(start[n], P)]
    lr = torch.stack([ref[n, c - 1] for n, c in rows])
    le = torch.stack([emu[n, c - 1] for n, c in rows])
    t = torch.stack([ids[n, c] for n, c in rows])
    lp, rank = S.token_stats(lr, t)
    lpe, ranke = S.token_stats(le, t)
    tol = 2.0 * float((le - lr).abs().max())
    near = ((lr - lr[torch.arange(len(rows)), t][:, None]).abs() <= tol).sum(1) - 1
    return dict(lp=lp, rank=rank, lp_emu=lpe, rank_emu=ranke, near=near, tol=tol)


def _stats_gate(what, lp, rank, o):
    """Log-prob vector: relative L2 <= 2 x the emulation's drift of the same vector.  Rank: off by at most the number of oracle logits
    within twice the emulation's largest absolute logit error of the target's (loose on random weights; exactness is test 1's job)."""
    assert torch.isfinite(lp).all() and bool((lp <= 0).all())
    _drift.check(f"{what} log-prob", L.rel(lp, o["lp"]), L.rel(o["lp_emu"], o["lp"]))
    drank = (rank.long() - o["rank"].long()).abs()
    print(f"    {what}: ranks moved on {int((drank > 0).sum())} of {len(drank)} rows (the emulation's own: "
          f"{int((o['rank_emu'] != o['rank']).sum())}), logit tolerance {o['tol']:.2e}")
    assert bool((drank <= o["near"]).all()), (drank.tolist(), o["near"].tolist())


@pytest.mark.parametrize("name", ["wide", "tiny"])
def test_handle_against_the_oracle(lms, name):
    """N = 2, lengths (64, 41) left-padded to P = 64, start (40, 50)."""
    lm = lms(name)
    P, start = 64, [40, 50]
    ids, first = L.left_padded((64, 41), P, L.CONFIGS[name].vocab_size, 2400)
    lp, rank = lm.score(ids.cuda(), L.mask_of(first, P).cuda(), start=start)
    assert lp.is_cuda and lp.shape == (sum(P - s for s in start),) and rank.dtype == torch.int32
    lp2, rank2 = lm.score(ids, L.mask_of(first, P), start=start)
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(rank, rank2)
    _stats_gate(f"{name} score", lp.cpu(), rank.cpu(), _oracle_stats(name, ids, first, start))


def test_score_leaves_no_generation(lms):
    """After score a decode raises, an older cache token is stale, and a following prefill has the bits of one on a fresh handle."""
    lm, fresh = lms("tiny"), lms("tiny", fresh=True)
    V = L.TINY.vocab_size
    ids, first = L.left_padded((30, 12), 30, V, 2404)
    mask = L.mask_of(first, 30)
    out = lm(input_ids=ids.cuda(), attention_mask=mask.cuda())
    lm.score(ids, mask, start=20)
    assert lm.length == 0
    with pytest.raises(ValueError, match="LM decode without a prefill"):
        lm.decode(torch.tensor([1, 2]))
    with pytest.raises(NotImplementedError, match="stale cache token"):
        lm(input_ids=torch.tensor([[1], [2]]).cuda(), past_key_values=out.past_key_values)
    from ace355 import native
    logits = torch.empty(2, V, device=lm.device)
    assert lm._lib.ace355_lm_decode(lm._h, (C.c_int32 * 2)(1, 2), native.ptr(logits), None) == 1 and "no prefill" in native.last_error()
    a = lm.prefill(ids, mask)
    b = fresh.prefill(ids, mask)
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(lm.decode(torch.tensor([3, 4]))), _bits(fresh.decode(torch.tensor([3, 4]))))


def test_handle_refusals_before_any_launch(gpu_device, lms):
    from ace355 import native
    from ace355.lm import NativeCausalLM
    lm = lms("tiny")
    V = L.TINY.vocab_size
    ids, first = L.left_padded((30, 12), 30, V, 2405)
    mask = L.mask_of(first, 30)
    keep = lm.prefill(ids, mask)
    gen = lm._generation
    for start in ([18, 18], [30, 20], [20, 30], [0, 20], [20], 30):   # first = (0, 18): start must lie in (first, P)
        with pytest.raises(ValueError, match="start"):
            lm.score(ids, mask, start=start)
    bad = ids.clone()
    bad[1, 25] = V
    with pytest.raises(ValueError, match="outside"):
        lm.score(bad, mask, start=20)
    with pytest.raises(ValueError, match="exceeds the handle"):
        lm.score(torch.zeros(5, 30, dtype=torch.int64), None, start=20)
    with pytest.raises(NotImplementedError, match="left-padded"):
        lm.score(ids, mask.flip(1), start=20)
    assert lm._generation == gen and lm.length == 30, "a refused score touched the generation"
    assert lm.decode(torch.tensor([3, 4])).shape == keep.shape

    # the library's own checks, below the Python layer
    p32 = C.POINTER(C.c_int32)
    lp = torch.empty(64, device=gpu_device)
    rank = torch.empty(64, dtype=torch.int32, device=gpu_device)

    def raw(h, idl, fl, sl, N, P):
        a, f, s = (C.c_int32 * len(idl))(*idl), (C.c_int32 * len(fl))(*fl), (C.c_int32 * len(sl))(*sl)
        return lm._lib.ace355_lm_score(h, C.cast(a, p32), C.cast(f, p32), C.cast(s, p32), N, P, native.ptr(lp), native.ptr(rank), None)

    flat = [int(v) for v in ids.flatten()]
    lm.prefill(ids, mask)
    assert raw(lm._h, flat, [0, 18], [20, 18], 2, 30) == 1 and "start[1] = 18" in native.last_error()
    assert raw(lm._h, flat, [0, 18], [30, 20], 2, 30) == 1 and "start[0] = 30" in native.last_error()
    assert raw(lm._h, flat[:-1] + [V], [0, 18], [20, 20], 2, 30) == 1 and "token id" in native.last_error()
    assert raw(lm._h, flat, [0, 30], [20, 20], 2, 30) == 1 and "first[1]" in native.last_error()
    assert raw(lm._h, flat, [0] * 5, [20] * 5, 5, 30) == 1 and "max_seqs" in native.last_error()
    assert lm.length == 30, "a refused ace355_lm_score dropped the generation"
    big = NativeCausalLM(L.TINY, gpu_device, max_positions=native.LM_MAX_POSITIONS, max_seqs=16)
    try:
        n_tok = 16 * 4097
        assert n_tok > native.LM_MAX_TOKENS
        assert raw(big._h, [0] * 8, [0] * 16, [1] * 16, 16, 4097) == 3 and "finalize" in native.last_error()   # unfinalized: refused first
        big.load_state_dict(dict(L.weights("tiny")))
        zeros = (C.c_int32 * n_tok)()
        f, s = (C.c_int32 * 16)(), (C.c_int32 * 16)(*([1] * 16))
        rc = big._lib.ace355_lm_score(big._h, C.cast(zeros, p32), C.cast(f, p32), C.cast(s, p32), 16, 4097, native.ptr(lp), native.ptr(rank), None)
        assert rc == 1 and "N * P" in native.last_error()
    finally:
        big.close()


# ------------------------------------------------------------------------------------------------ 5. the seam
def test_seam_on_the_recorded_request(lms, monkeypatch):
    """``lmscore.calculate_pmi_score_per_condition`` on a handler whose ``llm`` is a bare NativeCausalLM: G24's keys, per-token
    statistics within test 2's gates of G24's (transformers in fp32), scores equal to the CPU glue applied to the native statistics."""
    from ace355 import lmscore
    G = S.load_g24()
    lm = lms("tiny")
    tok = S.ToyTokenizer(L.TINY.vocab_size)
    rq = S.request(tok)
    h = S.FakeHandler(lm, tok, device="cuda", prompts=rq["prompts"])
    h.use_native_lm_score = True
    assert lmscore.native_lm(h) is lm
    seen = []
    inner = lmscore.target_stats
    monkeypatch.setattr(lmscore, "target_stats", lambda *a: seen.append(inner(*a)) or seen[-1])
    monkeypatch.setattr(lmscore, "_reference", lambda: None)   # no fallback: a native failure must show
    scores, global_score, status = lmscore.calculate_pmi_score_per_condition(h, rq["audio_codes"], caption=rq["caption"],
                                                                             lyrics=rq["lyrics"], metadata=dict(rq["metadata"]))
    assert sorted(scores) == [str(k) for k in G["req_keys"]], status
    assert len(seen) == int(G["req_n_calls"]) and h.context_entries == len(seen)
    for k, (lp, rank) in enumerate(seen):
        ids, plen = torch.from_numpy(G[f"req{k}_ids"]).long()[None], int(G[f"req{k}_plen"])
        assert lp.device.type == "cpu" and lp.shape == (ids.shape[1] - plen,)
        o = _oracle_stats("tiny", ids, [0], [plen])
        assert L.rel(o["lp"], torch.from_numpy(G[f"req{k}_lp"])) < 1e-5   # the oracle composition is transformers' forward
        o["lp"], o["rank"] = torch.from_numpy(G[f"req{k}_lp"]), torch.from_numpy(G[f"req{k}_rank"])
        _stats_gate(f"seam forward {k}", lp, rank, o)
    # the glue on the native statistics, restated: recall for the two fields, normalised PMI for caption and lyrics
    want = {"bpm": lmscore.topk_recall_of(seen[0][1])[0], "keyscale": lmscore.topk_recall_of(seen[1][1])[0],
            "caption": lmscore._own_pmi_to_normalized_score(lmscore.log_prob_of(seen[2][0]) - lmscore.log_prob_of(seen[3][0]), 0.1),
            "lyrics": lmscore._own_pmi_to_normalized_score(lmscore.log_prob_of(seen[4][0]) - lmscore.log_prob_of(seen[5][0]), 0.1)}
    assert scores == want
    assert global_score == lmscore._own_calculate_reward_score(want)[0]
    for key, g in zip(G["req_keys"], G["req_scores"]):
        print(f"    seam {key}: native {scores[str(key)]:.6f}, recorded {float(g):.6f}")
