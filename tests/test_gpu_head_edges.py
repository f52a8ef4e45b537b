"""The criterion, matcher and post-processing kernels on the MI355X at their edges: vrd_criterion_costs / _losses / _backward
(through losses.device_criterion, and the cost kernel called directly), vrd_assign (ops.assign) and vrd_postprocess
(ops.postprocess) against the float64 references, case tables, tolerances and checkers of tests/head_cases.py.

Every element of every output is compared; costs and gradients relative to their own (pair, query) row.  The bound of each
output kind is 8 E, E being the distance of the float32 tensor form from float64 over the whole table (head_cases.criterion_E /
post_E) -- nothing here is tuned to what the kernels return.  Each test prints its distances as fractions of the bound."""
import pytest
import torch

import head_cases as H
from vrdone_amd.models import losses as LS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def device_costs(inp):
    """vrd_criterion_costs called directly: cost (L, G, Q), which device_criterion does not return"""
    from vrdone_amd import _hip
    from vrdone_amd.ops import _stream
    L, G, Q = inp["L"], inp["G"], inp["Q"]
    keep = dict(logits=[t.to(DEV).contiguous() for t in inp["logits"]], masks=[t.to(DEV).contiguous() for t in inp["masks"]],
                valid=inp["valid"].to(DEV).contiguous().view(torch.uint8), owner=inp["owner"].to(DEV, torch.int32),
                ids=inp["ids"].to(DEV).long(), tgt=inp["tgt"].to(DEV).contiguous(),
                segs=inp["segs"].to(DEV, torch.int32).contiguous() if inp["fuzzy"] else None)
    a = _hip.CriterionArgs()
    for l in range(L):
        a.logits[l], a.masks[l] = keep["logits"][l].data_ptr(), keep["masks"][l].data_ptr()
    a.n_layers, a.B, a.Q, a.K1, a.T, a.G = L, inp["B"], Q, inp["K1"], inp["T"], G
    a.out_valid, a.tgt_ids, a.tgt_masks, a.owner = (keep[k].data_ptr() for k in ("valid", "ids", "tgt", "owner"))
    a.segs = keep["segs"].data_ptr() if inp["fuzzy"] else None
    a.scale_range = float(inp["scale_range"]) if inp["fuzzy"] else 1.0
    a.alpha, a.gamma = float(inp["alpha"]), float(inp["gamma"])
    a.w_class, a.w_mask, a.w_dice = (float(w) for w in inp["cost_w"])
    cost = torch.full((L, G, Q), float("nan"), device=DEV)
    _hip.check(_hip.lib.vrd_criterion_costs(_hip.C.byref(a), cost.data_ptr(), _stream()), "vrd_criterion_costs")
    torch.cuda.synchronize()
    return cost.cpu()


def device_criterion(inp):
    layers = [(lg.to(DEV).requires_grad_(True), mk.to(DEV).requires_grad_(True)) for lg, mk in zip(inp["logits"], inp["masks"])]
    with torch.enable_grad():
        vals, q_of, failed = LS.device_criterion(layers, inp["valid"].to(DEV), inp["sizes"], inp["ids"].to(DEV), inp["tgt"].to(DEV),
                                                 inp["segs"].to(DEV) if inp["fuzzy"] else None, inp["scale_range"], inp["weight"],
                                                 inp["cost_w"], alpha=inp["alpha"], gamma=inp["gamma"])
        (vals * inp["coef"].to(DEV)).sum().backward()
    assert not bool(failed)
    return {"loss": vals.detach().cpu(), "q_of": q_of.cpu(), "glogit": torch.stack([lg.grad for lg, _ in layers]).cpu(),
            "gmask": torch.stack([mk.grad for _, mk in layers]).cpu()}


@pytest.mark.parametrize("i", range(len(H.CRITERION_CASES)), ids=[H.case_id(c) for c in H.CRITERION_CASES])
def test_criterion_kernels_against_float64(i):
    """Costs, assignment, losses and both gradients of one case: per element against float64 within 8 E, all finite, scipy's
    assignment on the float64 costs (either of two that tie within the cost bound), exact zeros in the mask gradient of unmatched rows and invalid frames."""
    inp, ref = H.criterion_case(i)
    bound = H.criterion_bound()
    got = device_criterion(inp)
    got["cost"] = device_costs(inp)
    H.check_criterion(got, ref, inp, bound, label="HEAD-EDGES criterion " + H.case_id(H.CRITERION_CASES[i]))


@pytest.mark.parametrize("kind,Q", H.ASSIGN_CASES, ids=[f"{k}-Q{q}" for k, q in H.ASSIGN_CASES])
def test_assignment_on_tied_quantised_extreme_and_infinite_costs(kind, Q):
    """vrd_assign on the blocks early training produces -- queries that price a relation identically, quantised costs, 1e30 /
    1e-30 scales, +inf entries with and without a complete assignment left, a padded cost buffer -- against scipy: complete,
    injective, scipy's float64 total, scipy's very queries where the optimum is unique, -1 where scipy refuses the block."""
    from vrdone_amd import ops
    cost, sizes = H.assign_inputs(kind, Q)
    expect = H.assign_expect(cost, sizes)
    G, ld = cost.shape[0], cost.stride(0)
    buf = torch.full((G, ld), float("nan"), device=DEV)
    buf[:, :Q] = cost.to(DEV)
    got = ops.assign(buf[:, :Q], sizes)
    torch.cuda.synchronize()
    assert (ld > Q) == (kind == "ld") and got.dtype == torch.int32 and got.shape == (G,)
    H.check_assignment(got.cpu().numpy(), cost, sizes, expect, exact_sum=(kind == "int"))


@pytest.mark.parametrize("i", range(len(H.POST_SHAPES)), ids=["K{}-top{}-P{}xQ{}-T{}".format(*s) for s in H.POST_SHAPES])
def test_postprocess_classes_scores_and_segments(i):
    """vrd_postprocess at the lane / register boundaries of its class layout, on tied, underflowing, background-led and
    non-finite logit rows and on mask rows at the edges of the valid length: see head_cases.check_postprocess.  A row without a
    softmax returns NaN scores for distinct foreground classes and disturbs nothing else."""
    from vrdone_amd import ops
    inp, ref = H.post_case(i)
    bound = H.KERNEL_FACTOR * H.post_E()

    def run(logits):
        out = ops.postprocess(logits.to(DEV).contiguous(), inp["masks"].to(DEV).contiguous(), inp["valid_len"].to(DEV), inp["topk"])
        torch.cuda.synchronize()
        return tuple(t.cpu() for t in out)

    got = run(inp["logits"])
    worst = H.check_postprocess(got, inp, ref, bound)
    print("\nHEAD-EDGES postprocess", H.POST_SHAPES[i], f"score={worst / bound:.3f}")
    bad = ref["nonfinite"].view(inp["P"], inp["Q"])
    if bool(bad.any()):
        # the same call with finite logits in those rows: every other row's classes and scores, and all segments, bit for bit
        clean = inp["logits"].clone()
        clean[bad] = torch.randn(int(bad.sum()), inp["K1"], generator=torch.Generator().manual_seed(i))
        other = run(clean)
        assert torch.equal(got[0][~bad], other[0][~bad]) and torch.equal(got[1][~bad], other[1][~bad])
        assert torch.equal(got[2], other[2]) and torch.equal(got[3], other[3])
        H.check_postprocess(other, dict(inp, logits=clean), H.post_reference(dict(inp, logits=clean)), bound)
