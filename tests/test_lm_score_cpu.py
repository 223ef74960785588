"""CPU: the LM-score plan (csrc/lm_plan.h through the C ABI), the ``ace355.lmscore`` glue on fixture G24's recorded per-token statistics,
its routing rules, the ``get_hf_model_for_scoring`` override, and the refusals of ``NativeCausalLM.score`` - none of which needs a GPU."""
import logging
import os
import sys
import types

import pytest
import torch

import _lm_oracle as L
import _lm_score_ref as S


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("D", [256, 1024, 2048])
@pytest.mark.parametrize("V", [1003, 2051, 217205])
def test_plan_cuts_the_vocabulary_exactly_once_and_the_workspace_suffices(V, D):
    from ace355 import native
    first = native.lm_score_plan(1, V, D)
    for R in range(1, 301):
        p = native.lm_score_plan(R, V, D)
        chunk, chunks = p["chunk"], p["chunks"]
        assert (chunk, chunks) == (first["chunk"], first["chunks"]), "the cut of the vocabulary must not depend on R"
        # chunk c = [c * chunk, min(V, (c + 1) * chunk)): non-empty, disjoint by construction, and the last one ends at V
        assert chunk > 0 and (chunks - 1) * chunk < V <= chunks * chunk
        assert p["tile_rows"] > 0 and p["grid_x"] == -(-R // p["tile_rows"]) and p["grid_y"] == chunks
        # thresholds fp32 [R] + one 32-byte partial per (row, chunk), each region 256-byte aligned
        need = -(-R * 4 // 256) * 256 + -(-R * chunks * 32 // 256) * 256
        assert native.lm_score_workspace_bytes(R, V) == need >= R * 4 + R * chunks * 32


def test_plan_refuses_what_the_rows_entry_refuses():
    from ace355 import native
    for R, V, D in [(0, 1003, 256), (native.LM_MAX_TOKENS + 1, 1003, 256), (4, 0, 256), (4, (1 << 20) + 1, 256), (4, 1003, 0), (4, 1003, 96),
                    (4, 1003, 16384 + 64)]:
        with pytest.raises(RuntimeError, match="lm_score_plan"):
            native.lm_score_plan(R, V, D)
    assert native.lm_score_workspace_bytes(0, 1003) == 0 and native.lm_score_workspace_bytes(4, 0) == 0
    assert native.lm_score_plan(native.LM_MAX_TOKENS, 1 << 20, 16384)["chunks"] == 1024


def test_rows_entry_refuses_without_a_gpu():
    """Every refusal of ace355_lm_score_rows comes before its first HIP call."""
    from ace355 import native
    lib = native.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = native.ptr(buf)
    need = native.lm_score_workspace_bytes(4, 1003)
    assert lib.ace355_lm_score_rows(p, 256, None, p, p, 4, 1003, 256, p, p, p, need - 1, None) == 1
    assert "workspace of" in native.last_error() and str(need) in native.last_error()
    assert lib.ace355_lm_score_rows(p, 256, None, p, p, 4, 1003, 250, p, p, p, need, None) == 1
    assert lib.ace355_lm_score_rows(p, 255, None, p, p, 4, 1003, 256, p, p, p, need, None) == 1
    assert lib.ace355_lm_score_rows(None, 256, None, p, p, 4, 1003, 256, p, p, p, need, None) == 1
    assert lib.ace355_lm_score_rows(p + 2, 256, None, p, p, 4, 1003, 256, p, p, p, need, None) == 1 and "aligned" in native.last_error()


# ------------------------------------------------------------------------------------------------ the glue on recorded statistics
@pytest.fixture(scope="module")
def G():
    return S.load_g24()


def test_g24_holds_what_the_tests_rely_on(G):
    for i, (P, T, _seed) in enumerate(S.PAIRS):
        rank = G[f"pair{i}_rank"]
        assert int(G[f"pair{i}_plen"]) == P and rank.shape == (T,) and sorted(set(rank.tolist())) == list(range(min(T, S.RANK_CYCLE)))
        assert 0.0 < float(G[f"pair{i}_recall_avg"]) < 1.0
    assert int(G["req_n_calls"]) == 6 and [str(k) for k in G["req_keys"]] == ["bpm", "caption", "keyscale", "lyrics"]
    assert os.path.getsize(S.G24) < 64 * 1024


def test_pair_statistics_give_the_reference_numbers(G):
    from ace355 import lmscore
    for i in range(int(G["n_pairs"])):
        lp, rank = torch.from_numpy(G[f"pair{i}_lp"]), torch.from_numpy(G[f"pair{i}_rank"])
        assert lmscore.log_prob_of(lp) == float(G[f"pair{i}_mean_lp"])
        avg, per_k = lmscore.topk_recall_of(rank, 10)
        assert avg == float(G[f"pair{i}_recall_avg"])
        assert [per_k[k] for k in range(1, 11)] == G[f"pair{i}_recall_per_k"].tolist()
    assert lmscore.log_prob_of(torch.empty(0)) == float("-inf") and lmscore.topk_recall_of(torch.empty(0, dtype=torch.int32)) == (0.0, {})
    assert lmscore.topk_recall_of(torch.tensor([0, 9, 10, 3]), 10) == ((1.0 + 0.1 + 0.0 + 0.7) / 4, {**{k: 0.25 for k in (1, 2, 3)}, **{k: 0.5 for k in range(4, 10)}, 10: 0.75})


def _recorded_stats(G, tok, seen):
    """A ``target_stats`` that replays G24's forwards in the order the reference made them, checking the text it is handed."""
    def fake(handler, prompt, target):
        k = len(seen)
        ids = tok.encode(prompt + target)
        assert ids == G[f"req{k}_ids"].tolist() and len(tok.encode(prompt)) == int(G[f"req{k}_plen"]), f"forward {k}: other text than recorded"
        seen.append(k)
        return torch.from_numpy(G[f"req{k}_lp"]), torch.from_numpy(G[f"req{k}_rank"])
    return fake


def test_request_glue_reproduces_the_reference_exactly(G, monkeypatch):
    """Scores, global score and status string of the reference's calculate_pmi_score_per_condition, from its per-token statistics
    alone - with this package's own restatement of pmi_to_normalized_score / calculate_reward_score (the reference does not import)."""
    from ace355 import lmscore
    tok = S.ToyTokenizer(L.TINY.vocab_size)
    rq = S.request(tok)
    h = S.FakeHandler(object(), tok, prompts=rq["prompts"])
    seen = []
    monkeypatch.setattr(lmscore, "native_lm", lambda handler: object())
    monkeypatch.setattr(lmscore, "_reference", lambda: None)
    monkeypatch.setattr(lmscore, "target_stats", _recorded_stats(G, tok, seen))
    meta = dict(rq["metadata"])
    scores, global_score, status = lmscore.calculate_pmi_score_per_condition(h, rq["audio_codes"], caption=rq["caption"],
                                                                             lyrics=rq["lyrics"], metadata=meta)
    assert seen == list(range(6)) and meta["caption"] == rq["caption"]
    assert sorted(scores) == [str(k) for k in G["req_keys"]]
    assert [scores[str(k)] for k in G["req_keys"]] == G["req_scores"].tolist()
    assert global_score == float(G["req_global"])
    assert status == str(G["req_status"])


def test_restated_arithmetic():
    from ace355 import lmscore
    assert lmscore._own_pmi_to_normalized_score(0.0) == 0.5
    assert lmscore._own_pmi_to_normalized_score(0.1, 0.1) == pytest.approx(1 / (1 + 2.718281828459045 ** -1))
    assert lmscore._own_calculate_reward_score({}) == (0.0, "❌ No valid scores available to calculate reward.")
    total, text = lmscore._own_calculate_reward_score({"lyrics": 0.5, "bpm": 1.0, "genres": 0.0})   # no caption: 0.3 and 0.2 renormalised
    assert total == pytest.approx(0.5 * 0.6 + 0.5 * 0.4)
    assert text.splitlines() == ["  • Lyrics   | Score: 0.5000 | Weight: 0.60 -> Contrib: +0.3000",
                                 "  • Metadata | Score: 0.5000 | Weight: 0.40 -> Contrib: +0.2000"]


# ------------------------------------------------------------------------------------------------ routing
def _bare_lm():
    """A NativeCausalLM without a handle: enough for isinstance and for the checks score() makes before its native call."""
    from ace355.lm import NativeCausalLM
    lm = NativeCausalLM.__new__(NativeCausalLM)
    lm.cfg, lm.max_seqs, lm.max_positions, lm.device = L.TINY, 4, 128, torch.device("cpu")
    lm._generation, lm._first = 5, [0]
    return lm


def _handler(llm, flag=True, backend="pt"):
    h = S.FakeHandler(llm, S.ToyTokenizer(L.TINY.vocab_size), prompts={"cond": "", "uncond": ""})
    h.use_native_lm_score = flag
    h.llm_backend = backend
    return h


def test_native_path_is_taken_only_under_all_three_rules():
    from ace355 import lmscore, modswap
    lm = _bare_lm()
    swap = modswap.NativeCausalLMSwap(lm, torch.nn.Identity(), "llm")
    assert lmscore.native_lm(_handler(lm)) is lm
    assert lmscore.native_lm(_handler(swap)) is lm
    assert lmscore.native_lm(types.SimpleNamespace(llm=lm, use_native_lm_score=True)) is lm   # llm_backend absent
    assert lmscore.native_lm(_handler(lm, flag=False)) is None
    assert lmscore.native_lm(_handler(lm, backend="vllm")) is None
    assert lmscore.native_lm(_handler(lm, backend="mlx")) is None
    assert lmscore.native_lm(_handler(torch.nn.Identity())) is None
    assert lmscore.native_lm(_handler(None)) is None
    plain = types.SimpleNamespace(llm=lm)                                  # no flag attribute at all
    assert lmscore.native_lm(plain) is None


def _fake_reference(monkeypatch, calls):
    """A stand-in acestep.core.scoring.lm_score that records what reaches it."""
    ref = types.ModuleType("acestep.core.scoring.lm_score")

    def rec(name, ret):
        def f(*a, **k):
            calls.append((name, a, k))
            return ret
        return f
    ref._calculate_log_prob = rec("_calculate_log_prob", -1.5)
    ref._calculate_topk_recall = rec("_calculate_topk_recall", (0.25, {1: 0.0}))
    ref._calculate_metadata_recall = rec("_calculate_metadata_recall", {"bpm": 0.5})
    ref.calculate_pmi_score_per_condition = rec("calculate_pmi_score_per_condition", ({"caption": 0.5}, 0.5, "ref status"))
    ref.pmi_to_normalized_score = lambda pmi, scale=0.1: 0.125
    ref.calculate_reward_score = lambda scores, weights_config=None: (0.75, "ref breakdown")
    for name in ("acestep", "acestep.core", "acestep.core.scoring"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    sys.modules["acestep.core.scoring"].lm_score = ref
    monkeypatch.setitem(sys.modules, "acestep.core.scoring.lm_score", ref)
    return ref


def test_calls_off_the_native_path_run_the_reference(monkeypatch):
    from ace355 import lmscore
    calls = []
    _fake_reference(monkeypatch, calls)
    monkeypatch.setattr(lmscore, "target_stats", lambda *a: (_ for _ in ()).throw(AssertionError("the native path must not be taken")))
    h = _handler(_bare_lm(), flag=False)
    assert lmscore.calculate_log_prob(h, "p", "t") == -1.5
    assert lmscore.calculate_topk_recall(h, "p", "t", topk=7) == (0.25, {1: 0.0})
    assert lmscore.calculate_metadata_recall(h, "p", {"bpm": 1}) == {"bpm": 0.5}
    meta = {"bpm": 1}
    assert lmscore.calculate_pmi_score_per_condition(h, "codes", caption="c", lyrics="l", metadata=meta, topk=3) == ({"caption": 0.5}, 0.5, "ref status")
    assert [c[0] for c in calls] == ["_calculate_log_prob", "_calculate_topk_recall", "_calculate_metadata_recall",
                                     "calculate_pmi_score_per_condition"]
    assert calls[1][2] == {"topk": 7} and calls[3][1] == (h, "codes") and calls[3][2]["metadata"] is meta and calls[3][2]["topk"] == 3
    assert calls[3][2]["caption"] == "c" and calls[3][2]["lyrics"] == "l" and calls[3][2]["score_scale"] == 0.1
    assert meta == {"bpm": 1}, "off the native path the arguments reach the reference untouched"
    # the arithmetic is the host's when it imports
    assert lmscore.pmi_to_normalized_score(3.0) == 0.125 and lmscore.calculate_reward_score({"caption": 1.0}) == (0.75, "ref breakdown")


def test_a_native_failure_runs_the_reference_and_is_logged_three_times(monkeypatch, caplog):
    from ace355 import lmscore
    calls = []
    _fake_reference(monkeypatch, calls)
    monkeypatch.setattr(lmscore, "_failures", 0)

    def boom(*a):
        raise RuntimeError("ace355 native call failed (lm_score)")
    monkeypatch.setattr(lmscore, "target_stats", boom)
    h = _handler(_bare_lm())
    with caplog.at_level(logging.WARNING, logger="ace355"):
        for _ in range(3):
            assert lmscore.calculate_pmi_score_per_condition(h, "codes", caption="c", metadata={"bpm": 1}) == ({"caption": 0.5}, 0.5, "ref status")
        assert lmscore.calculate_log_prob(h, "p", "t") == -1.5
        assert lmscore.calculate_topk_recall(h, "p", "t") == (0.25, {1: 0.0})
    assert len(calls) == 5
    assert sum("[native-lm-score]" in r.getMessage() for r in caplog.records) == 3


def test_without_the_reference_the_error_payload_comes_back(monkeypatch):
    from ace355 import lmscore
    monkeypatch.setattr(lmscore, "_reference", lambda: None)
    monkeypatch.setattr(lmscore, "_failures", 0)
    monkeypatch.setattr(lmscore, "target_stats", lambda *a: (_ for _ in ()).throw(RuntimeError("device lost")))
    h = _handler(_bare_lm())
    assert lmscore.calculate_pmi_score_per_condition(h, "codes", caption="c", metadata={}) == ({}, float("-inf"), "❌ Error: device lost")
    with pytest.raises(RuntimeError, match="device lost"):
        lmscore.calculate_log_prob(h, "p", "t")
    off = _handler(_bare_lm(), flag=False)
    scores, score, status = lmscore.calculate_pmi_score_per_condition(off, "codes", caption="c", metadata={})
    assert scores == {} and score == float("-inf") and status.startswith("❌ Error: ")
    with pytest.raises(RuntimeError, match="does not import"):
        lmscore.calculate_topk_recall(off, "p", "t")


def test_native_path_keeps_the_reference_s_early_answers(monkeypatch):
    from ace355 import lmscore
    monkeypatch.setattr(lmscore, "_reference", lambda: None)
    monkeypatch.setattr(lmscore, "target_stats", lambda *a: (torch.empty(0), torch.empty(0, dtype=torch.int32)))
    h = _handler(_bare_lm())
    assert lmscore.calculate_pmi_score_per_condition(h, "  ", metadata={}) == ({}, 0.0, "❌ No audio codes provided")
    h.llm_initialized = False
    assert lmscore.calculate_pmi_score_per_condition(h, "codes", metadata={}) == ({}, 0.0, "❌ LLM not initialized")
    h.llm_initialized = True
    assert lmscore.calculate_pmi_score_per_condition(h, "codes", metadata={"caption": None}) == ({}, 0.0, "❌ No conditions to evaluate")


def test_an_empty_target_makes_no_native_call():
    from ace355 import lmscore
    lm = _bare_lm()
    lm.score = lambda *a, **k: (_ for _ in ()).throw(AssertionError("no native call for an empty target"))
    h = _handler(lm)
    lp, rank = lmscore.target_stats(h, h.llm_tokenizer.text([1, 2, 3]), "")
    assert lp.shape == (0,) and lp.dtype == torch.float32 and rank.shape == (0,) and rank.dtype == torch.int32
    assert h.context_entries == 0
    assert lmscore._native_log_prob(h, "abc", "") == float("-inf") and lmscore._native_topk_recall(h, "abc", "") == (0.0, {})


def test_target_stats_scores_the_full_text_from_the_prompt_length():
    from ace355 import lmscore
    lm = _bare_lm()
    got = {}

    def score(ids, mask, start):
        got.update(ids=ids.tolist(), mask=mask.tolist(), start=start)
        return torch.tensor([-1.0, -2.0]), torch.tensor([0, 4], dtype=torch.int32)
    lm.score = score
    h = _handler(lm)
    lp, rank = lmscore.target_stats(h, h.llm_tokenizer.text([1, 2, 3]), h.llm_tokenizer.text([16, 17]))
    assert got == {"ids": [[1, 2, 3, 16, 17]], "mask": [[1] * 5], "start": 3} and h.context_entries == 1
    assert lp.tolist() == [-1.0, -2.0] and rank.tolist() == [0, 4]


# ------------------------------------------------------------------------------------------------ the mixin
def test_flag_default_and_scoring_model_override():
    from ace355 import backend, modswap
    assert backend.NativeLmMixin.use_native_lm_score is (os.environ.get("ACE355_LM_SCORE", "") == "1")

    class Base:
        def get_hf_model_for_scoring(self):
            return "the host's answer"

    class Host(backend.NativeLmMixin, Base):
        pass

    kept = torch.nn.Identity()
    h = Host()
    h.llm, h.llm_backend = modswap.NativeCausalLMSwap(_bare_lm(), kept, "llm"), "pt"
    assert h.get_hf_model_for_scoring() is kept
    del h.llm_backend                                     # absent: the reference's own default is "pt"
    assert h.get_hf_model_for_scoring() is kept
    h.llm_backend = "vllm"
    assert h.get_hf_model_for_scoring() == "the host's answer"
    h.llm, h.llm_backend = kept, "pt"                     # no swap installed
    assert h.get_hf_model_for_scoring() == "the host's answer"
    h.llm = None
    assert h.get_hf_model_for_scoring() == "the host's answer"


# ------------------------------------------------------------------------------------------------ refusals of NativeCausalLM.score
def test_score_refuses_before_any_native_call():
    """Where prefill refuses, and for a start outside (first, P); a refusal leaves the generation alone.  (The bare object has no
    library and sits on the CPU: reaching the native call fails on that, with no ace355 refusal.)"""
    lm = _bare_lm()
    V = L.TINY.vocab_size
    ids = torch.zeros(2, 30, dtype=torch.int64)
    mask = L.mask_of([0, 18], 30)
    for bad, exc in [(dict(ids=torch.zeros(30, dtype=torch.int64), start=20), ValueError),
                     (dict(ids=torch.zeros(2, 0, dtype=torch.int64), start=20), ValueError),
                     (dict(ids=ids, start=None), ValueError),
                     (dict(ids=ids, attention_mask=mask, start=[18, 18]), ValueError),
                     (dict(ids=ids, attention_mask=mask, start=[20, 30]), ValueError),
                     (dict(ids=ids, attention_mask=mask, start=[20]), ValueError),
                     (dict(ids=ids, start=0), ValueError),
                     (dict(ids=ids, start=30), ValueError),
                     (dict(ids=ids + V, start=20), ValueError),
                     (dict(ids=ids.float(), start=20), ValueError),
                     (dict(ids=torch.zeros(5, 30, dtype=torch.int64), start=20), ValueError),
                     (dict(ids=torch.zeros(2, 129, dtype=torch.int64), start=20), ValueError),
                     (dict(ids=ids, attention_mask=mask[:, :29], start=20), NotImplementedError),
                     (dict(ids=ids, attention_mask=mask.flip(1), start=20), NotImplementedError),
                     (dict(ids=ids, attention_mask=torch.zeros(2, 30, dtype=torch.int64), start=20), NotImplementedError)]:
        with pytest.raises(exc, match="ace355"):
            lm.score(**bad)
    assert lm._generation == 5 and lm._first == [0]
    with pytest.raises((AttributeError, ValueError), match="cuda device|_lib"):
        lm.score(ids, mask, start=[19, 19])   # a valid request gets as far as the native call
    assert lm._generation == 6 and lm._first is None
    with pytest.raises(ValueError, match="LM decode without a prefill"):
        lm.decode(torch.tensor([1]))
