"""tests/head_cases.py without a GPU: the case tables cover what they claim, the float64 references agree with the golden-pinned
forms, the tolerances come out of the table, and the checkers reject stand-ins of the faults the GPU tests exist for."""
import math

import numpy as np
import pytest
import torch

import head_cases as H
from oracle import vrd_oracle as O
from vrdone_amd.models import losses as LS


def by_name(name, fuzzy):
    return next(i for i, c in enumerate(H.CRITERION_CASES) if c["name"] == name and c["fuzzy"] == fuzzy)


# ------------------------------------------------------------------------------------------------------- the tables
def test_criterion_table_covers_the_listed_shapes_and_values():
    cases = H.CRITERION_CASES
    hard = [c for c in cases if not c["fuzzy"]]
    assert len(cases) == 2 * len(hard) and all(dict(c, fuzzy=True) in cases for c in hard)            # hard and fuzzy throughout
    assert {1, 9, 16} <= {c["Q"] for c in cases}
    assert {2, 51, 64, 65, 133} <= {c["K1"] for c in cases}
    assert {1, 63, 64, 65, 96, 200} <= {c["T"] for c in cases}
    assert {1, 4} <= {c["L"] for c in cases}
    G = {sum(c["sizes"]) for c in cases}
    assert {1, 63, 64, 65} <= G and any(1000 <= g <= 1200 for g in G)
    big = [c for c in cases if sum(c["sizes"]) >= 1000 and c["B"] == 130]
    assert big and all(c["Q"] == 9 for c in big)
    assert {(c["B"] * c["Q"], c["Q"]) for c in cases} >= {(12222, 9), (12224, 16)}
    assert 4 * 12224 + 16 * 4 * 4 <= 48 * 1024 < 4 * 12225 + 16 * 4 * 4            # 12,224 rows are the last that fit
    assert 4 * (1359 * 9) + 256 > 48 * 1024                                        # and one more pair of 9 queries does not
    assert {(c["alpha"], c["gamma"]) for c in cases} == set(H.ALPHA_GAMMA) and all(c["gamma"] >= 1 for c in cases)
    assert {2.0, 30.0, 100.0} <= {c["mask_scale"] for c in cases} and {1.0, 50.0} <= {c["logit_scale"] for c in cases}
    assert {0.85, 1.0} <= {c["scale_range"] for c in cases if c["fuzzy"] and c["segs"] == "edges"}
    assert {"random", "eos"} <= {c["weights"] for c in cases}
    # pairs without relations between pairs with Q relations
    assert any(any(a == c["Q"] and b == 0 and d == c["Q"] for a, b, d in zip(c["sizes"], c["sizes"][1:], c["sizes"][2:])) for c in cases)
    # valid lengths 1, T and every residue mod 64
    lens = [(n, c["T"]) for c in cases for n in c["lens"]]
    assert {n % 64 for n, _ in lens} == set(range(64)) and any(n == 1 for n, _ in lens) and any(n == T for n, T in lens)


def test_criterion_inputs_hold_the_planted_values_and_boundary_segments():
    inp, _ = H.criterion_case(by_name("planted", True))
    x = torch.stack(inp["masks"])[:, inp["valid"][:, None, :].expand(-1, inp["Q"], -1)]
    for v in H.PLANTED:
        assert bool((x == torch.tensor(v)).any()), v
    assert bool((x > 20).any()) and bool((x.abs() > 88.8).any())                    # softplus' linear branch; expf overflow
    inp, _ = H.criterion_case(by_name("mask100", False))
    assert float(torch.stack(inp["masks"]).abs().max()) > 200
    inp, _ = H.criterion_case(by_name("seg_edges", True))
    segs, n = inp["segs"], torch.tensor([96, 96, 50])[inp["owner"]]
    assert {int(d) for d in segs[:, 1] - segs[:, 0]} == {1, 20, 40, 60, 80}
    assert bool((segs[:, 0] == 0).any()) and bool((segs[:, 1] == n).any())
    assert bool(((segs[:, 1] == n) & (n < inp["T"])).any())                          # a widened ramp reaching past the valid length
    # a frame exactly on the core boundary: |off| == length / 2 * scale_range in f32, and the target jumps there
    lo, hi = segs[:, 0], segs[:, 1]
    off = (torch.arange(inp["T"], dtype=torch.float32)[None] - ((hi - 1 + lo).float() / 2)[:, None]).abs()
    edge = off == ((hi - lo)[:, None] / 2 * 0.85)
    assert {int(d) for d in (hi - lo)[edge.any(-1)]} == {20, 60} and int(edge.sum()) == 14          # both ends of 7 segments
    tp = H.fuzzy_targets64(inp["tgt"], segs, inp["valid"][inp["owner"]], 0.85)
    on_edge = tp[edge & inp["valid"][inp["owner"]]]
    assert bool((on_edge < 0.7).all()) and bool((on_edge > 0.6).all())
    # per-layer coefficients and class weights are arbitrary
    assert inp["coef"].unique().numel() == inp["coef"].numel() and inp["weight"].unique().numel() > 2


def test_assignment_table_covers_the_listed_blocks():
    assert {Q for _, Q in H.ASSIGN_CASES} == {1, 2, 9, 16} and {k for k, _ in H.ASSIGN_CASES} == set(H.ASSIGN_KINDS)
    refused = solved = ambiguous = 0
    for kind, Q in H.ASSIGN_CASES:
        cost, sizes = H.assign_inputs(kind, Q)
        assert len(sizes) > 64 and set(sizes) == set(range(Q + 1)) and cost.shape == (sum(sizes), Q) and cost.dtype == torch.float32
        exp = H.assign_expect(cost, sizes)
        if kind == "int":
            assert set(cost.unique().tolist()) == {0.0, 1.0, 2.0, 3.0}
        if kind == "identical_columns" and Q > 1:
            assert torch.equal(cost[:, 0], cost[:, 1])
        if kind == "base_noise" and Q > 1:
            assert float((cost - cost[:, :1]).abs().max()) < 1e-6
        if kind.startswith("scale_"):
            assert (float(cost.abs().max()) > 1e30) == (kind == "scale_1e30") and bool(torch.isfinite(cost).all())
            assert float(cost.abs().max()) > 1e-30 and bool((cost != 0).all())
        if kind == "ld":
            assert cost.stride(0) > Q
        if kind == "inf40":
            assert 0.3 < float(torch.isinf(cost).float().mean()) < 0.6 and not bool((cost == -math.inf).any())
            assert sum(e is None for e in exp) >= 10 and sum(e is not None and len(e[0]) >= 1 for e in exp) >= 10         # at every Q
            refused += sum(e is None for e in exp)
            solved += sum(e is not None and len(e[0]) for e in exp)
        else:
            assert all(e is not None for e in exp)
        if kind in ("random", "ld", "scale_1e30", "scale_1e-30"):
            assert all(e[2] for e in exp), kind                                       # continuous costs: the optimum is unique
        ambiguous += sum(e is not None and not e[2] for e in exp)
    assert refused > 20 and solved > 20 and ambiguous > 100


def test_postprocess_table_covers_the_listed_shapes_and_rows():
    S = H.POST_SHAPES
    assert {2, 3, 17, 51, 64, 65, 128, 129, 133, 255, 256} == {s[0] for s in S}
    assert {1, 6, 8, 16} <= {s[1] for s in S} and {(2, 1), (3, 2), (17, 16)} <= {(s[0], s[1]) for s in S}         # topk = K1 - 1
    assert {1, 63, 64, 70} == {s[2] * s[3] for s in S} and {1, 63, 64, 65, 96, 512} == {s[4] for s in S}
    lk, mk, vl = set(), set(), set()
    for i, s in enumerate(S):
        inp, ref = H.post_case(i)
        lk |= set(inp["lkind"])
        mk |= set(inp["mkind"])
        vl |= {int(v) - s[4] if v >= s[4] else int(v) for v in inp["valid_len"]}
        x = inp["masks"]
        assert not bool(((x != 0) & (x.abs() < 2.0 ** -20)).any())                   # there f32 sigmoid rounds to 0.5
        rows = inp["logits"].view(-1, s[0])
        for r, k in enumerate(inp["lkind"]):
            assert bool(ref["nonfinite"][r]) == (k in H.NONFINITE_KINDS), (s, r, k)
            if k == "x100":
                assert int((ref["probs"][r].float() == 0).sum()) >= s[0] // 3 or s[0] <= 3         # exact ties at 0
            if k == "bg_max":
                assert int(rows[r].argmax()) == 0
            if isinstance(k, tuple):
                assert int(rows[r].argmax()) == k[1]
            if k == "dup_top" and s[0] > 2:
                assert int((rows[r] == rows[r].max()).sum()) >= 2
    assert lk == set(H.LOGIT_KINDS) | {("max_at", c) for c in H.MAX_AT} and mk == set(H.MASK_KINDS)
    assert {0, 1, 5} <= vl                                                             # 0, 1, T (= 0 past T), T + 5
    # every non-finite kind also meets topk = K1 - 1, where the kernel runs out of comparable candidates
    inp, _ = H.post_case(S.index((17, 16, 8, 8, 65)))
    assert set(H.NONFINITE_KINDS) <= set(inp["lkind"])


# --------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("name,T", [("vidvrd", 96), ("vidor_x", 512)])
def test_float64_criterion_form_equals_the_oracle_on_the_golden_inputs(name, T):
    mc, pred, (gp, gm, gs), inp = H.golden_criterion(name, T)
    want, idx = O.criterion(mc, pred, gp, gm, gs)
    got = H.criterion_form(inp, torch.float64)
    lf = mc["loss_coeff_dict"]
    for l, suffix in enumerate(["", "_0", "_1", "_2"]):
        for i, k in enumerate(("loss_class", "loss_mask", "loss_dice")):
            w, g = float(want[k + suffix]), lf[k] * float(got["loss"][l, i])
            assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (k + suffix, g, w)
    at = 0
    for (qs, js), n in zip(idx, inp["sizes"]):                                        # the final layer's matches
        assert got["q_of"][0, at + torch.as_tensor(js)].tolist() == list(map(int, qs))
        at += n


def test_fuzzy_target_membership_is_the_tensor_forms():
    """fuzzy_targets64 decides core / ramp exactly as losses.fuzzy_targets does, and differs from it only by f32 rounding of
    the ramp; the float32 form of the criterion is losses.py as it stands."""
    for name in ("seg_edges", "seg_edges_sr1", "q9_l4", "residues_t200"):
        inp, _ = H.criterion_case(by_name(name, True))
        vo = inp["valid"][inp["owner"]]
        a = LS.fuzzy_targets(inp["tgt"], inp["segs"], vo, inp["scale_range"])
        b = H.fuzzy_targets64(inp["tgt"], inp["segs"], vo, inp["scale_range"])
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(a == 0, b == 0) and torch.equal(a == 1, b == 1)
        assert float((a.double() - b).abs().max()) < 1e-3 and float((a.double() - b).abs().mean()) < 1e-6
    inp, _ = H.criterion_case(by_name("seg_edges_sr1", True))
    assert torch.equal(H.fuzzy_targets64(inp["tgt"], inp["segs"], inp["valid"][inp["owner"]], 1.0), inp["tgt"].double())


def test_tolerances_come_from_the_table_and_the_f32_form_sits_inside_them():
    E, bound = H.criterion_E(), H.criterion_bound()
    print("criterion E:", E)
    for k in H.KINDS:
        assert 0 < E[k] < 1e-3 and bound[k] == 8 * E[k], (k, E[k])                    # f32 rounding, not a lost term
    worst = dict.fromkeys(H.KINDS, 0.0)
    for i, c in enumerate(H.CRITERION_CASES):
        inp, ref = H.criterion_case(i)
        d = H.check_criterion(H.criterion_form(inp, torch.float32, q_of=ref["q_of"]), ref, inp, bound)
        worst = {k: max(worst[k], d[k]) for k in H.KINDS}
        for k in ("glogit", "gmask"):
            assert bool(torch.isfinite(ref[k]).all())
    assert all(worst[k] * H.KERNEL_FACTOR <= bound[k] for k in H.KINDS)
    pE = H.post_E()
    print("postprocess E:", pE)
    assert 0 < pE < 1e-5
    for i in range(len(H.POST_SHAPES)):
        inp, ref = H.post_case(i)
        assert H.check_postprocess(H.post_emulation(inp), inp, ref, H.KERNEL_FACTOR * pE) * H.KERNEL_FACTOR <= H.KERNEL_FACTOR * pE


# ----------------------------------------------------------------------------------------- the checkers reject faults
CRITERION_FAULTS = [("k65_t65", H.fault_last_stride_dropped, "cost: .* from float64"), ("q9_l4", H.fault_valid_ignored, "cost: .* from float64"),
                    ("planted", H.fault_softplus_without_linear_branch, "non-finite"),
                    ("q9_l4", H.fault_class_weights_ignored, "loss: .* from float64"), ("g65", H.fault_first_ballot_round_only, "gmask: .* from float64"),
                    ("g1089", H.fault_first_ballot_round_only, "gmask: .* from float64"),
                    ("q9_l4", H.fault_small_gradient_on_unmatched_row, "non-zero entries on unmatched")]


@pytest.mark.parametrize("fuzzy", [False, True])
@pytest.mark.parametrize("name,fault,message", CRITERION_FAULTS, ids=[f.__name__ + "-" + n for n, f, _ in CRITERION_FAULTS])
def test_criterion_checker_rejects(name, fault, message, fuzzy):
    inp, ref = H.criterion_case(by_name(name, fuzzy))
    bound = H.criterion_bound()
    H.check_criterion(H.criterion_form(inp, torch.float32, q_of=ref["q_of"]), ref, inp, bound)
    got = fault(inp, ref)
    with pytest.raises(AssertionError, match=message):
        H.check_criterion(got, ref, inp, bound)
    if fault is H.fault_small_gradient_on_unmatched_row:
        # ... which the tensor-relative comparison of tests/test_gpu_train.py lets through
        assert float((got["gmask"].double() - ref["gmask"]).abs().max()) <= 1e-6 * max(1.0, float(ref["gmask"].abs().max())) + 1e-7


def test_criterion_checker_takes_either_assignment_of_identical_relations_only():
    """Two relations of a pair with the same class and segment cost the same with every query: the kernels may give them each
    other's queries.  Any other exchange is an assignment that differs."""
    inp, ref = H.criterion_case(by_name("g63", False))
    bound = H.criterion_bound()
    same = [(a, b) for a in range(inp["G"]) for b in range(a + 1, inp["G"]) if inp["owner"][a] == inp["owner"][b]
            and inp["ids"][a] == inp["ids"][b] and torch.equal(inp["segs"][a], inp["segs"][b])]
    other = [(a, b) for a in range(inp["G"] - 1) for b in [a + 1] if inp["owner"][a] == inp["owner"][b] and inp["ids"][a] != inp["ids"][b]]
    assert same and other
    for (a, b), fine in ((same[0], True), (other[0], False)):
        q = ref["q_of"].clone()
        q[0, a], q[0, b] = ref["q_of"][0, b], ref["q_of"][0, a]
        got = H.criterion_form(inp, torch.float32, q_of=q)
        if fine:
            H.check_criterion(got, ref, inp, bound)
        else:
            with pytest.raises(AssertionError, match="assignment differs"):
                H.check_criterion(got, ref, inp, bound)


def test_assignment_checker_rejects_a_repeated_query_and_a_dearer_assignment():
    cost, sizes = H.assign_inputs("int", 9)
    exp = H.assign_expect(cost, sizes)
    good = np.concatenate([e[0] for e in exp])
    H.check_assignment(good, cost, sizes, exp, exact_sum=True)
    first = np.cumsum([0] + sizes)
    p = next(p for p, n in enumerate(sizes) if n == 5)
    twice = good.copy()
    twice[first[p] + 1] = twice[first[p]]
    with pytest.raises(AssertionError, match="not distinct"):
        H.check_assignment(twice, cost, sizes, exp, exact_sum=True)
    # one unit dearer: move a relation to a free query that costs exactly 1 more
    blk = cost[first[p]:first[p] + 5].numpy()
    free = sorted(set(range(9)) - set(good[first[p]:first[p] + 5].tolist()))
    i, j = next((i, j) for i in range(5) for j in free if blk[i, j] == blk[i, good[first[p] + i]] + 1)
    dearer = good.copy()
    dearer[first[p] + i] = j
    with pytest.raises(AssertionError, match="optimum"):
        H.check_assignment(dearer, cost, sizes, exp, exact_sum=True)
    # a pair scipy refuses must come back -1 throughout, a pair it solves must not
    cost, sizes = H.assign_inputs("inf40", 2)
    exp = H.assign_expect(cost, sizes)
    first = np.cumsum([0] + sizes)
    good = np.concatenate([e[0] if e is not None else np.full(n, -1) for e, n in zip(exp, sizes)])
    H.check_assignment(good, cost, sizes, exp)
    p = next(p for p, e in enumerate(exp) if e is None)
    bad = good.copy()
    bad[first[p]] = 0
    with pytest.raises(AssertionError, match="refuses"):
        H.check_assignment(bad, cost, sizes, exp)
    p = next(p for p, e in enumerate(exp) if e is not None and len(e[0]))
    bad = good.copy()
    bad[first[p]] = -1
    with pytest.raises(AssertionError, match="unassigned"):
        H.check_assignment(bad, cost, sizes, exp)


@pytest.mark.parametrize("fault,message", [(H.fault_background_returned, "category out of"), (H.fault_tie_to_higher_class, "higher class"),
                                           (H.fault_segment_includes_valid_len, "segments differ"),
                                           (H.fault_sentinel_category, "category out of")], ids=lambda f: getattr(f, "__name__", None))
def test_postprocess_checker_rejects(fault, message):
    i = H.POST_SHAPES.index((133, 8, 7, 9, 96))
    inp, ref = H.post_case(i)
    bound = H.KERNEL_FACTOR * H.post_E()
    H.check_postprocess(H.post_emulation(inp), inp, ref, bound)
    with pytest.raises(AssertionError, match=message):
        H.check_postprocess(fault(inp), inp, ref, bound)


def test_postprocess_checker_rejects_swapped_and_wrong_scores():
    inp, ref = H.post_case(H.POST_SHAPES.index((51, 6, 7, 10, 96)))
    bound = H.KERNEL_FACTOR * H.post_E()
    r = inp["lkind"].index("random")
    ts, tc, sf, sl = H.post_emulation(inp)
    ts.view(-1, 6)[r, :2] = ts.view(-1, 6)[r, :2].flip(0)
    with pytest.raises(AssertionError, match="descending"):
        H.check_postprocess((ts, tc, sf, sl), inp, ref, bound)
    ts, tc, sf, sl = H.post_emulation(inp)
    tc.view(-1, 6)[r, 5] = next(c for c in range(1, 51) if c not in tc.view(-1, 6)[r].tolist())          # a class that is not 6th
    with pytest.raises(AssertionError, match="from float64"):
        H.check_postprocess((ts, tc, sf, sl), inp, ref, bound)
    ts, tc, sf, sl = H.post_emulation(inp)
    ts.view(-1, 6)[inp["lkind"].index("nan")] = 0.25
    with pytest.raises(AssertionError, match="without a softmax"):
        H.check_postprocess((ts, tc, sf, sl), inp, ref, bound)
    assert math.isnan(float(H.post_emulation(inp)[0].view(-1, 6)[inp["lkind"].index("all_neg_inf"), 0]))
