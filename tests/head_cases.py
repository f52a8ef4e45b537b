"""Shared by tests/test_head_cases_cpu.py and tests/test_gpu_head_edges.py: the case tables, float64 references, tolerances and
checkers of the kernels that turn the head's logits into decisions -- vrd_criterion_costs / _losses / _backward
(csrc/vrd_criterion.hip), vrd_assign (csrc/vrd_train_tail.hip) and vrd_postprocess (csrc/vrd_post.hip) -- at the shapes and
values where such kernels go wrong, plus Python stand-ins of the faults the checkers exist for.  Nothing here needs a GPU.

References.  Criterion: the tensor forms of vrdone_amd/models/losses.py (pair_costs, matched_losses) and F.cross_entropy on
float64 CPU tensors, gradients by autograd through them.  The fuzzy target's core / ramp membership is decided in float32 exactly
as losses.fuzzy_targets (and the reference) decides it -- a frame can sit exactly on a threshold --, its ramp value is then
evaluated in float64 (`fuzzy_targets64`), which is what oracle.vrd_oracle.relation_target does: the float64 form equals
oracle.criterion to 1e-12 (test_head_cases_cpu.py).  Assignment: scipy.optimize.linear_sum_assignment on the float64 image of
the f32 block.  Post-processing: float64 softmax with class 0 dropped; a frame is on iff its mask logit is > 0.

Tolerances.  None is a chosen number: for every output kind E is the largest distance, over the whole case table, of the SAME
tensor form evaluated in float32 on the CPU from the float64 form, and a kernel may be 8 E away (its sums run over 64 strided
lanes and a butterfly instead of torch's order, and device expf / logf / cosf are 1-2 ulp off).  Distances of costs and gradients
are relative to the largest reference entry of the element's own (pair, query) row, never to the tensor's."""
import functools
import json
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

from vrdone_amd.models import losses as LS

KERNEL_FACTOR = 8.0            # a kernel may be this many E from float64 (see the module docstring)

# ===================================================================================================== criterion
COST_W = (2.0, 5.0, 5.0)
KINDS = ("cost", "loss", "glogit", "gmask")
ALPHA_GAMMA = [(0.25, 2.0), (-1.0, 2.0), (0.25, 1.5), (-1.0, 3.0)]
PLANTED = [0.0, 20.0, -20.0, 20.0001, -20.0001, 88.0, -88.0, 104.0, -104.0]
# segments of 1, 20, 40, 60 and 80 frames, touching frame 0 and the last valid frame.  Frames sit at half-integer offsets from
# the centre of an even segment, and the core ends at length / 2 * 0.85: 8.5 and 25.5 for 20 and 60 frames -- a frame EXACTLY on
# the boundary, where the target jumps from 1 to 0.65 --, 17 and 34 for 40 and 80, half a frame from the nearest one.  Pair 2
# has 50 valid frames of 96, so the widened ramp of (30, 50) reaches past them
EDGE_SEGS = [[(0, 1), (5, 25), (0, 40), (16, 96), (76, 96), (95, 96), (30, 70), (3, 83), (20, 80)],
             [(0, 20), (0, 80), (56, 96), (10, 11), (1, 21), (2, 42), (8, 88), (36, 96), (20, 60)],
             [(30, 50), (0, 1), (10, 50)]]


def _cycle(pattern, n):
    return [pattern[i % len(pattern)] for i in range(n)]


def _case(name, B, Q, K1, T, L, sizes, lens, **kw):
    d = dict(name=name, B=B, Q=Q, K1=K1, T=T, L=L, sizes=list(sizes), lens=list(lens), alpha=0.25, gamma=2.0, mask_scale=2.0,
             logit_scale=1.0, planted=False, segs="random", scale_range=0.85, weights="random")
    d.update(kw)
    assert len(d["sizes"]) == B and len(d["lens"]) == B and max(d["sizes"]) <= Q and 1 <= min(d["lens"]) and max(d["lens"]) <= T
    return d


def _base_cases():
    mid = dict(B=4, Q=9, K1=17, T=65, L=2, sizes=[9, 0, 3, 1], lens=[65, 64, 30, 1])
    c = [
        # ---- shapes: Q 1 / 9 / 16 (16 = 1024 threads per block of the cost kernel), K1, T, L
        _case("q1_t1", 5, 1, 2, 1, 1, [1, 0, 1, 1, 0], [1] * 5),
        _case("q9_l4", 7, 9, 51, 63, 4, [3, 1, 0, 9, 2, 4, 1], [63, 58, 40, 63, 17, 31, 3]),
        _case("q16", 6, 16, 64, 64, 1, [16, 0, 16, 5, 1, 0], [64, 64, 33, 1, 64, 20]),
        _case("k65_t65", 5, 9, 65, 65, 1, [9, 0, 9, 2, 1], [65, 64, 65, 1, 7]),
        _case("k133_t96", 4, 9, 133, 96, 4, [2, 9, 0, 3], [96, 91, 65, 50], weights="eos"),
        # ---- valid lengths 1, T and every residue mod 64
        _case("residues_t200", 66, 9, 5, 200, 1, _cycle([1, 0, 2], 66), [1, 200] + [64 + r for r in range(64)]),
        # ---- G around the 64-wide ballot of the backward kernel, and two rounds of the loss kernel's 1024-thread strides
        _case("g1", 2, 9, 3, 8, 1, [0, 1], [8, 5]),
        _case("g63", 8, 9, 3, 8, 1, [9] * 7 + [0], _cycle([8, 5, 1, 7], 8)),
        _case("g64", 8, 9, 3, 8, 1, [9] * 7 + [1], _cycle([8, 5, 1, 7], 8)),
        _case("g65", 8, 9, 3, 8, 1, [9] * 7 + [2], _cycle([8, 5, 1, 7], 8)),
        _case("g1089", 130, 9, 3, 8, 2, [0 if i % 16 == 1 else 9 for i in range(130)], _cycle([8, 5, 1, 7, 3], 130)),
        # ---- the last (pair, query) tables that fit the loss kernel's 48 KiB
        _case("rows12222", 1358, 9, 2, 2, 1, _cycle([1, 0, 0, 2, 0, 0, 0, 9], 1358), _cycle([2, 1], 1358)),
        _case("rows12224", 764, 16, 2, 2, 1, _cycle([1, 0, 0, 16, 0, 2], 764), _cycle([2, 1], 764)),
        # ---- magnitudes
        _case("mask30", **mid, mask_scale=30.0),
        _case("mask100", **mid, mask_scale=100.0),
        _case("planted", **mid, planted=True),
        _case("logit50", **mid, logit_scale=50.0),
        # ---- segments on the boundaries, and scale_range 1
        _case("seg_edges", 3, 9, 17, 96, 1, [9, 9, 3], [96, 96, 50], segs="edges"),
        _case("seg_edges_sr1", 3, 9, 17, 96, 1, [9, 9, 3], [96, 96, 50], segs="edges", scale_range=1.0),
    ]
    c += [_case(f"alpha{a:g}_gamma{g:g}", **mid, alpha=a, gamma=g) for a, g in ALPHA_GAMMA[1:]]
    return c


CRITERION_CASES = [dict(c, fuzzy=fz) for c in _base_cases() for fz in (False, True)]


def case_id(c):
    return c["name"] + ("-fuzzy" if c["fuzzy"] else "-hard")


def criterion_inputs(case):
    """The f32 CPU inputs of a case, as device_criterion takes them (plus owner, coef = d total / d loss[l][i])."""
    g = torch.Generator().manual_seed(zlib.crc32(case["name"].encode()) & 0xFFFF)
    B, Q, K1, T, L = (case[k] for k in ("B", "Q", "K1", "T", "L"))
    sizes, lens = case["sizes"], torch.tensor(case["lens"])
    G = sum(sizes)
    valid = torch.arange(T)[None] < lens[:, None]
    owner = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    ids = torch.randint(1, K1, (G,), generator=g)
    segs = torch.zeros(G, 2, dtype=torch.int64)
    if case["segs"] == "edges":
        segs = torch.tensor([s for pair in EDGE_SEGS for s in pair])
    else:
        for i in range(G):
            n = int(lens[owner[i]])
            a = int(torch.randint(0, max(n - 1, 1), (1,), generator=g))
            segs[i, 0], segs[i, 1] = a, int(torch.randint(a + 1, n + 1, (1,), generator=g))
    t = torch.arange(T)[None]
    tgt = ((t >= segs[:, :1]) & (t < segs[:, 1:])).float()
    logits, masks = [], []
    for _ in range(L):
        lg = torch.randn(B, Q, K1, generator=g) * case["logit_scale"]
        if case["logit_scale"] > 1:
            # keep a runner-up within 2 of every row's maximum: with one class alone at softmax = 1 - 1e-9 the row's whole
            # gradient is the cancellation 1 - p, which no f32 form resolves, and E would say nothing
            v, i = lg.topk(2, -1)
            lg.scatter_(-1, i[..., 1:], v[..., :1] - 2 * torch.rand(B, Q, 1, generator=g))
        mk = torch.randn(B, Q, T, generator=g) * case["mask_scale"]
        if case["mask_scale"] > 2:
            # frame 0 (always valid) stays moderate, for the same reason: a row saturated in every frame has no gradient in f32
            mk[..., 0] = 2 * torch.randn(B, Q, generator=g)
        if case["planted"]:
            pick = torch.randint(0, 3 * len(PLANTED), (B, Q, T), generator=g)
            pick[..., 0] = 3 * len(PLANTED) - 1
            mk = torch.where(pick < len(PLANTED), torch.tensor(PLANTED)[pick.clamp(max=len(PLANTED) - 1)], mk)
        logits.append(lg)
        masks.append(mk)
    weight = torch.ones(K1)
    weight[0] = 0.1
    if case["weights"] == "random":
        weight = 0.1 + 1.9 * torch.rand(K1, generator=g)
    return dict(B=B, Q=Q, K1=K1, T=T, L=L, G=G, sizes=sizes, valid=valid, owner=owner, ids=ids, segs=segs, tgt=tgt, logits=logits,
                masks=masks, weight=weight, cost_w=COST_W, coef=torch.randn(L, 3, generator=g), fuzzy=case["fuzzy"],
                scale_range=case["scale_range"], alpha=case["alpha"], gamma=case["gamma"])


def fuzzy_targets64(targets, segs, valid, scale_range):
    """losses.fuzzy_targets with the ramp in float64.  Which frames are core / ramp is decided by the very float32 expressions
    of losses.fuzzy_targets (checked against it in test_head_cases_cpu.py); off is a multiple of 0.5 and exact in both."""
    T = valid.shape[1]
    lo, hi = segs[:, 0], segs[:, 1]
    centre = (hi - 1 + lo).float() / 2
    off = torch.arange(T, dtype=torch.float32)[None, :] - centre[:, None]
    length = (hi - lo)[:, None]
    core = off.abs() < (length / 2 * scale_range)
    wide = (off.abs() < (length / 2 / scale_range)) & valid
    ramp = (wide ^ core) & valid
    w = torch.cos(math.pi / (length.double() / scale_range) * off.double())
    w = (w * (w > 0)) ** 0.5
    return w * ramp + targets.double() * core


def solve_pairs(cost, sizes):
    """scipy's assignment of every pair's block of cost (G, Q) -> query of every relation (G,) int64"""
    q = torch.zeros(cost.shape[0], dtype=torch.int64)
    at = 0
    for n in sizes:
        if n:
            rows, cols = linear_sum_assignment(cost[at:at + n].T.numpy())           # rows = queries, cols = relations
            q[at + torch.as_tensor(cols)] = torch.as_tensor(rows)
        at += n
    return q


def criterion_form(inp, dtype, q_of=None, valid=None, weight=None):
    """models/losses.py's tensor forms in `dtype` on the CPU: cost (L, G, Q), q_of (L, G) (scipy on these costs unless given),
    loss (L, 3) [class, focal, dice], glogit (L, B, Q, K1) and gmask (L, B, Q, T) = d sum(coef * loss) / d prediction.
    float32 is the form as it stands (what E measures); float64 takes the float64 ramp.  `valid` / `weight` replace the
    case's (the fault stand-ins)."""
    valid = inp["valid"] if valid is None else valid
    weight = (inp["weight"] if weight is None else weight).to(dtype)
    owner, ids, sizes, G = inp["owner"], inp["ids"], inp["sizes"], inp["G"]
    vo = valid[owner]
    if inp["fuzzy"] and dtype == torch.float64:
        tgt, soft = fuzzy_targets64(inp["tgt"], inp["segs"], vo, inp["scale_range"]), (None, None)
    else:
        tgt, soft = inp["tgt"].to(dtype), ((inp["segs"], inp["scale_range"]) if inp["fuzzy"] else (None, None))
    ag = dict(alpha=inp["alpha"], gamma=inp["gamma"])
    out = {k: [] for k in ("cost", "q_of", "loss", "glogit", "gmask")}
    for l in range(inp["L"]):
        lg = inp["logits"][l].to(dtype).clone().requires_grad_(True)
        mk = inp["masks"][l].to(dtype).clone().requires_grad_(True)
        with torch.no_grad():
            cc, cm, cd = LS.pair_costs(lg, mk, valid, ids, tgt, owner, *soft, **ag)
            cost = inp["cost_w"][0] * cc + inp["cost_w"][1] * cm + inp["cost_w"][2] * cd
        q = solve_pairs(cost, sizes) if q_of is None else q_of[l]
        with torch.enable_grad():                           # (a test module may have switched autograd off for the process)
            target = torch.zeros(inp["B"], inp["Q"], dtype=torch.int64)
            target[owner, q] = ids
            ce = F.cross_entropy(lg.transpose(1, 2), target, weight)
            focal, dice = LS.matched_losses(mk[owner, q], tgt, float(max(G, 1)), vo, *soft, **ag)
            loss = torch.stack([ce, focal, dice])
            (loss * inp["coef"][l].to(dtype)).sum().backward()
        for k, v in zip(out, (cost, q, loss.detach(), lg.grad, mk.grad)):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _cached(i):
    inp = criterion_inputs(CRITERION_CASES[i])
    ref = criterion_form(inp, torch.float64)
    return inp, ref


def criterion_case(i):
    """(inputs, float64 reference) of CRITERION_CASES[i]: built once, shared by every test, never written to."""
    return _cached(i)


def matched_rows(inp, q_of):
    """(L, B, Q) bool: the (pair, query) rows some relation was assigned to"""
    m = torch.zeros(q_of.shape[0], inp["B"], inp["Q"], dtype=torch.bool)
    for l in range(q_of.shape[0]):
        m[l, inp["owner"], q_of[l].long()] = True
    return m


def _row_distance(got, ref, den):
    """max |got - ref| / den; a row whose reference is all zero has to be zero"""
    err = (got.double() - ref.double()).abs()
    dead = (den == 0).expand_as(err)
    if bool((err[dead] != 0).any()):
        return math.inf
    return float((err / den.where(den > 0, torch.ones_like(den)))[~dead].max()) if bool((~dead).any()) else 0.0


def criterion_distances(got, ref, inp):
    """{kind: distance of got from ref}.  cost: relative to the largest reference cost of the entry's (pair, query) -- over the
    pair's relations; glogit / gmask: to the largest reference entry of the (pair, query) row; loss: to the value itself."""
    L, B, Q, owner = inp["L"], inp["B"], inp["Q"], inp["owner"]
    cden = torch.zeros(L, B, Q, dtype=torch.float64).scatter_reduce_(1, owner[None, :, None].expand(L, -1, Q), ref["cost"].abs().double(),
                                                                     "amax", include_self=True)
    return {"cost": _row_distance(got["cost"], ref["cost"], cden[:, owner]),
            "loss": _row_distance(got["loss"][..., None], ref["loss"][..., None], ref["loss"].abs().double()[..., None]),
            "glogit": _row_distance(got["glogit"], ref["glogit"], ref["glogit"].abs().amax(-1, keepdim=True).double()),
            "gmask": _row_distance(got["gmask"], ref["gmask"], ref["gmask"].abs().amax(-1, keepdim=True).double())}


@functools.lru_cache(maxsize=None)
def criterion_E():
    """{kind: E}: the largest distance of the float32 tensor form from the float64 one over CRITERION_CASES (same assignment)."""
    E = dict.fromkeys(KINDS, 0.0)
    for i in range(len(CRITERION_CASES)):
        inp, ref = criterion_case(i)
        d = criterion_distances(criterion_form(inp, torch.float32, q_of=ref["q_of"]), ref, inp)
        E = {k: max(E[k], d[k]) for k in KINDS}
    return E


def criterion_bound():
    return {k: KERNEL_FACTOR * v for k, v in criterion_E().items()}


def check_criterion(got, ref, inp, bound, valid=None, label=None):
    """got / ref: dicts of cost, q_of, loss, glogit, gmask.  Returns the distances; raises AssertionError on: a non-finite
    element, an assignment other than the reference's, a mask gradient that is not exactly 0.0 on an unmatched row or an
    invalid frame, a distance above bound[kind].  (An assignment that is not scipy's: see below.)"""
    problems = []
    for k in KINDS:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        if not bool(torch.isfinite(got[k]).all()):
            problems.append(f"{k}: {int((~torch.isfinite(got[k])).sum())} non-finite elements")
    if not torch.equal(got["q_of"].long(), ref["q_of"]):
        # The kernels assign on their own f32 costs, up to bound["cost"] of the row's largest from the float64 ones: where two
        # assignments of a pair are closer than that (identical relations of a pair are the common case) either is right.
        # Such a pair must be assigned completely, injectively and within that slack of the optimum; every other pair as scipy
        # does.  Losses and gradients are then compared with the float64 form OF THE ASSIGNMENT GIVEN.
        slack = 2 * inp["Q"] * bound["cost"]
        try:
            for l in range(inp["L"]):
                check_assignment(got["q_of"][l].numpy(), ref["cost"][l], inp["sizes"], assign_expect(ref["cost"][l], inp["sizes"], slack),
                                 slack=slack)
            ref = dict(criterion_form(inp, torch.float64, q_of=got["q_of"].long()), cost=ref["cost"])
        except AssertionError as e:
            problems.append(f"assignment differs from scipy's on the float64 costs: layer {l}, {e}")
    valid = inp["valid"] if valid is None else valid
    live = matched_rows(inp, ref["q_of"])[..., None] & valid[None, :, None, :]
    stray = got["gmask"][~live.expand_as(got["gmask"])]
    if not bool((stray == 0).all()):
        problems.append(f"gmask: {int((stray != 0).sum())} non-zero entries on unmatched rows / invalid frames")
    d = criterion_distances(got, ref, inp)
    if label:                                               # the distances as fractions of the bound, before anything is raised
        print(f"\n{label}", " ".join(f"{k}={d[k] / bound[k]:.3f}" for k in KINDS))
    problems += [f"{k}: {d[k]:.3e} from float64, bound {bound[k]:.3e}" for k in KINDS if not d[k] <= bound[k]]
    assert not problems, "; ".join(problems)
    return d


def golden_criterion(name, T):
    """(model config, stored predictions of the golden case, ground truth lists, the case as criterion inputs): the reference's
    own predictions of all four decoder layers, as tests/test_oracle_golden.py reads them."""
    from oracle.synth import synth_relations
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, f"state_keys_{name}.json")) as f:
        mc = json.load(f)["model_config"]
    with open(os.path.join(golden, f"criterion_{name}.json")) as f:
        seed = json.load(f)[f"T{T}"]["seed"]
    z = np.load(os.path.join(golden, f"mask_vrd_{name}.npz"))
    t = lambda k: torch.from_numpy(z[f"T{T}_{k}"])        # noqa: E731
    lens = z[f"T{T}_lengths"].tolist()
    valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    heads = [""] + [f"aux{i}_" for i in range(3)]
    pred = {"pred_logits": t("pred_logits"), "pred_masks": t("pred_masks"), "output_mask": valid[:, None, :],
            "aux_outputs": [{"pred_logits": t(h + "pred_logits"), "pred_masks": t(h + "pred_masks")} for h in heads[1:]]}
    gp, gm, gs = synth_relations(lens, T, mc["num_classes"], seed=seed)
    fuzzy = bool(mc.get("with_fuzzy", False))
    B, Q, K1 = pred["pred_logits"].shape
    sizes = [len(p) for p in gp]
    weight = torch.ones(K1, dtype=torch.float64)           # (eos_coef as the oracle holds it, not rounded to f32)
    weight[0] = mc["loss_coeff_dict"]["eos_coef"]
    cw = mc["cost_coeff_dict"]
    inp = dict(B=B, Q=Q, K1=K1, T=T, L=4, G=sum(sizes), sizes=sizes, valid=valid,
               owner=torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)), ids=torch.cat(gp).long(), segs=torch.cat(gs).long(),
               tgt=torch.cat(gm).float(), logits=[t(h + "pred_logits") for h in heads], masks=[t(h + "pred_masks") for h in heads],
               weight=weight, cost_w=(cw["cost_class"], cw["cost_mask"], cw["cost_dice"]), coef=torch.ones(4, 3), fuzzy=fuzzy,
               scale_range=mc.get("scale_range"), alpha=0.25, gamma=2.0)
    return mc, pred, (gp, gm, gs if fuzzy else None), inp


# ---------------------------------------------------------------------------------- criterion: stand-ins of faults
def fault_last_stride_dropped(inp, ref):
    """the frames of the last 64-stride (t >= 64 * ((T - 1) // 64)) never visited"""
    valid = inp["valid"].clone()
    valid[:, 64 * ((inp["T"] - 1) // 64):] = False
    return criterion_form(inp, torch.float32, q_of=ref["q_of"], valid=valid)


def fault_valid_ignored(inp, ref):
    return criterion_form(inp, torch.float32, q_of=ref["q_of"], valid=torch.ones_like(inp["valid"]))


def fault_softplus_without_linear_branch(inp, ref):
    """log1p(exp(x)) for every x: exp overflows above 88.7 and the cost of every relation of the pair is infinite"""
    got = criterion_form(inp, torch.float32, q_of=ref["q_of"])
    x = torch.stack(inp["masks"])
    extra = ((torch.log1p(torch.exp(x)) - F.softplus(x)) * inp["valid"][None, :, None, :]).sum(-1)          # (L, B, Q)
    got["cost"] = got["cost"] + inp["cost_w"][1] * extra[:, inp["owner"]]
    return got


def fault_class_weights_ignored(inp, ref):
    return criterion_form(inp, torch.float32, q_of=ref["q_of"], weight=torch.ones_like(inp["weight"]))


def fault_first_ballot_round_only(inp, ref):
    """a row matched to relation 64 or later is taken for unmatched: no mask gradient"""
    got = criterion_form(inp, torch.float32, q_of=ref["q_of"])
    for l in range(inp["L"]):
        got["gmask"][l, inp["owner"][64:], ref["q_of"][l, 64:]] = 0.0
    return got


def fault_small_gradient_on_unmatched_row(inp, ref):
    """one unmatched row gets a gradient of 1e-6 of the tensor's largest entry: invisible to a tensor-relative comparison"""
    got = criterion_form(inp, torch.float32, q_of=ref["q_of"])
    free = (~matched_rows(inp, ref["q_of"])).nonzero()
    l, b, q = free[len(free) // 2].tolist()
    got["gmask"][l, b, q, 0] = 1e-6 * float(ref["gmask"].abs().max())
    return got


# ===================================================================================================== assignment
ASSIGN_Q = (1, 2, 9, 16)
ASSIGN_KINDS = ("random", "int", "identical_columns", "base_noise", "scale_1e30", "scale_1e-30", "inf40", "ld")
ASSIGN_CASES = [(kind, Q) for kind in ASSIGN_KINDS for Q in ASSIGN_Q]


def assign_inputs(kind, Q):
    """(cost (G, Q) f32 -- a view of a wider buffer for "ld" --, sizes): every N <= Q, more than 64 pairs"""
    g = torch.Generator().manual_seed(zlib.crc32(f"{kind}{Q}".encode()) & 0xFFFF)
    sizes = [n for _ in range(-(-65 // (Q + 1))) for n in range(Q + 1)]
    G = sum(sizes)
    cost = torch.randn(G, Q, generator=g)
    if kind == "int":
        cost = torch.randint(0, 4, (G, Q), generator=g).float()
    elif kind == "identical_columns":                       # queries that price every relation identically, two by two
        cost[:, 1::2] = cost[:, 0:Q - 1:2]
    elif kind == "base_noise":                              # a relation costs the same with every query, to the last few ulp
        cost = (torch.randn(G, 1, generator=g).double() + 1e-7 * torch.randn(G, Q, generator=g).double()).float()
    elif kind.startswith("scale_"):
        cost = cost * float(kind[6:])
    elif kind == "inf40":
        cost[torch.rand(G, Q, generator=g) < 0.4] = math.inf
        at = 0
        for p, n in enumerate(sizes):                       # and blocks without a complete assignment at every Q:
            if p % 5 == 3 and n >= 2:                       # two relations that only query p % Q can take
                keep = cost[at:at + 2, p % Q].clamp(max=9.0).clone()
                cost[at:at + 2] = math.inf
                cost[at:at + 2, p % Q] = keep
            if p % 5 == 4 and n >= 1:                       # a relation no query can take
                cost[at + n - 1] = math.inf
            at += n
    elif kind == "ld":
        buf = torch.full((G, Q + 3), math.nan)
        buf[:, :Q] = cost
        cost = buf[:, :Q]
    return cost, sizes


def _chosen_sum(blk, q):
    return float(blk[np.arange(len(q)), q].sum())


def assign_expect(cost, sizes, margin=1e-9):
    """per pair: None when scipy refuses the block (NaN / -inf entry, or no complete assignment over the finite entries), else
    (scipy's query per relation, float64 sum of the chosen entries, whether the optimum is unique -- every other assignment dearer
    by more than `margin` of the block's largest finite |cost| --, that largest |cost|)"""
    out, at = [], 0
    for n in sizes:
        blk = cost[at:at + n].double().numpy()
        at += n
        if n == 0:
            out.append((np.zeros(0, dtype=np.int64), 0.0, True, 0.0))
            continue
        try:
            rows, cols = linear_sum_assignment(blk.T)
        except ValueError:
            out.append(None)
            continue
        q = np.empty(n, dtype=np.int64)
        q[cols] = rows
        best = _chosen_sum(blk, q)
        # unique iff forbidding any one chosen entry makes the optimum strictly worse
        unique, scale = True, float(np.abs(blk[np.isfinite(blk)]).max())
        for i in range(n):
            alt = blk.copy()
            alt[i, q[i]] = math.inf
            try:
                r2, c2 = linear_sum_assignment(alt.T)
            except ValueError:
                continue
            if alt[c2, r2].sum() - best <= margin * scale:
                unique = False
                break
        out.append((q, best, unique, scale))
    return out


def check_assignment(got, cost, sizes, expect, exact_sum=False, slack=0.0):
    """got (G,) int: raises AssertionError unless every pair scipy solves is assigned completely, to distinct queries, at
    scipy's float64 total (exactly for integer costs, to 1e-12 otherwise; `slack` of the block's largest |cost| more when the
    assignment was made on costs that far from `cost`) and to scipy's very queries where the optimum is unique, and every pair
    scipy refuses is -1 throughout."""
    got = np.asarray(got, dtype=np.int64)
    Q, at = cost.shape[1], 0
    for p, (n, exp) in enumerate(zip(sizes, expect)):
        mine = got[at:at + n]
        blk = cost[at:at + n].double().numpy()
        at += n
        if exp is None:
            assert (mine == -1).all(), f"pair {p}: scipy refuses this block, got {mine.tolist()}"
            continue
        q, best, unique, scale = exp
        assert ((mine >= 0) & (mine < Q)).all(), f"pair {p}: unassigned or out of range {mine.tolist()}"
        assert len(set(mine.tolist())) == n, f"pair {p}: queries not distinct {mine.tolist()}"
        total = _chosen_sum(blk, mine)
        assert total == best if exact_sum else abs(total - best) <= 1e-12 * abs(best) + slack * scale, f"pair {p}: total {total!r}, optimum {best!r}"
        if unique:
            assert (mine == q).all(), f"pair {p}: unique optimum {q.tolist()}, got {mine.tolist()}"


# ================================================================================================ post-processing
# (K1, topk, P, Q, T): K1 around the lane / register boundaries of the class layout (class c = lane c % 64, register c / 64),
# topk 1 .. 16 and K1 - 1, P * Q in {1, 63, 64, 70} (70 = a tail block of 2 rows), T around the 64-frame stride
POST_SHAPES = [(2, 1, 7, 9, 63), (3, 2, 7, 10, 1), (3, 1, 1, 1, 64), (17, 16, 8, 8, 65), (17, 6, 7, 9, 96), (51, 6, 7, 10, 96),
               (64, 8, 7, 9, 64), (65, 16, 7, 10, 65), (128, 8, 8, 8, 63), (129, 16, 7, 10, 512), (133, 8, 7, 9, 96),
               (255, 16, 7, 10, 65), (256, 16, 7, 10, 96), (256, 1, 7, 9, 1)]
MAX_AT = (1, 63, 64, 65, 127, 128, 191, 192, 255)
LOGIT_KINDS = ("random", "x100", "dup_top", "all_equal", "bg_max", "neg_inf_subset", "nan", "pinf", "all_neg_inf")
NONFINITE_KINDS = ("nan", "pinf", "all_neg_inf")
MASK_KINDS = ("random", "all_off", "all_on", "first", "last_valid", "at_valid_len", "f63", "f64", "f65", "pm_zero", "pm_inf",
              "nan_frame")
SURE_UNDERFLOW = -110.0        # expf(x) is 0 in f32 for x < -103.98 with or without denormals: below -110 two classes surely tie


def post_inputs(shape):
    """logits (P, Q, K1), masks (P, Q, T), valid_len (P,) int32, topk and the kind of every (pair, query) row"""
    K1, topk, P, Q, T = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr(shape).encode()) & 0xFFFF)
    PQ = P * Q
    logits = torch.randn(PQ, K1, generator=g) * 2
    masks = torch.randn(PQ, T, generator=g) * 3
    valid_len = torch.tensor([[0, 1, T, T + 5][p] if p < 4 else int(torch.randint(1, T + 1, (1,), generator=g)) for p in range(P)],
                             dtype=torch.int32)
    if P == 1:
        valid_len[0] = T
    lkinds = list(LOGIT_KINDS) + [("max_at", c) for c in MAX_AT if c < K1]
    lkind, mkind = [], []
    for r in range(PQ):
        lk = lkinds[r % len(lkinds)] if PQ > 1 else "random"
        mk = MASK_KINDS[(5 * r + 3) % len(MASK_KINDS)] if PQ > 1 else "random"
        row, m = logits[r], masks[r]
        fg = 1 + (r * 7) % (K1 - 1)                       # a foreground class that moves with the row
        if lk == "x100":
            row *= 50.0                                    # 2 * 50: most probabilities underflow to exactly 0
        elif lk == "dup_top":
            row[torch.randperm(K1 - 1, generator=g)[:3] + 1] = float(row.max()) + 1.0
        elif lk == "all_equal":
            row[:] = 0.7
        elif lk == "bg_max":
            row[0] = float(row.max()) + 10.0
        elif lk == "neg_inf_subset":
            row[torch.rand(K1, generator=g) < 0.5] = -math.inf
            row[fg] = 0.3
        elif lk == "nan":
            row[fg] = math.nan
        elif lk == "pinf":
            row[fg] = math.inf
        elif lk == "all_neg_inf":
            row[:] = -math.inf
        elif isinstance(lk, tuple):
            row[lk[1]] = float(row.max()) + 5.0
        n = min(int(valid_len[r // Q]), T)
        if mk != "random":
            m[:] = torch.where(torch.rand(T, generator=g) < 0.5, 3.0, -3.0) if mk in ("pm_inf", "nan_frame") else -3.0
        if mk == "all_on":
            m[:] = 3.0
        elif mk == "first":
            m[0] = 3.0
        elif mk == "last_valid" and n >= 1:
            m[n - 1] = 3.0
        elif mk == "at_valid_len" and n < T:
            m[n] = 3.0
        elif mk in ("f63", "f64", "f65") and int(mk[1:]) < T:
            m[int(mk[1:])] = 3.0
        elif mk == "pm_zero":
            m[:] = torch.where(torch.rand(T, generator=g) < 0.5, 0.0, -0.0)
        elif mk == "pm_inf":
            m[torch.rand(T, generator=g) < 0.3] = math.inf
            m[torch.rand(T, generator=g) < 0.3] = -math.inf
        elif mk == "nan_frame":
            m[r % T] = math.nan
        lkind.append(lk)
        mkind.append(mk)
    return dict(K1=K1, topk=topk, P=P, Q=Q, T=T, logits=logits.view(P, Q, K1), masks=masks.view(P, Q, T), valid_len=valid_len,
                lkind=lkind, mkind=mkind)


def post_reference(inp):
    """float64: probs (PQ, K1), the top-k foreground values (PQ, topk), which rows have no softmax (a NaN / +inf logit, or all
    -inf), and [first, last] frame with mask logit > 0 inside min(valid_len, T), -1 / -1 when there is none"""
    P, Q, K1, T = inp["P"], inp["Q"], inp["K1"], inp["T"]
    lg = inp["logits"].view(P * Q, K1).double()
    probs = torch.softmax(lg, -1)
    nonfinite = torch.isnan(probs).any(-1)
    vals = torch.topk(torch.nan_to_num(probs[:, 1:], nan=0.0), inp["topk"], dim=-1).values
    n = inp["valid_len"].long().clamp(max=T).repeat_interleave(Q)
    on = (inp["masks"].view(P * Q, T) > 0) & (torch.arange(T)[None] < n[:, None])
    idx = torch.arange(T)[None].expand_as(on)
    first = torch.where(on, idx, T).amin(-1)
    last = torch.where(on, idx, -1).amax(-1)
    return dict(probs=probs, vals=vals, nonfinite=nonfinite, first=torch.where(last < 0, -1, first), last=last)


@functools.lru_cache(maxsize=None)
def post_case(i):
    inp = post_inputs(POST_SHAPES[i])
    return inp, post_reference(inp)


@functools.lru_cache(maxsize=None)
def post_E():
    """largest distance of f32 torch.softmax from the float64 one over the table's finite rows, relative to the row's largest
    probability"""
    E = 0.0
    for i in range(len(POST_SHAPES)):
        inp, ref = post_case(i)
        p32 = torch.softmax(inp["logits"].view(-1, inp["K1"]), -1).double()
        ok = ~ref["nonfinite"]
        E = max(E, float(((p32 - ref["probs"]).abs() / ref["probs"].amax(-1, keepdim=True))[ok].max()))
    return E


def post_emulation(inp):
    """The kernel's contract in f32 torch on the CPU (stable descending sort = ties to the lower class; a row without a softmax
    returns NaN scores for the lowest foreground classes): what the checker must accept, and the base of the fault stand-ins."""
    P, Q, K1, T, k = inp["P"], inp["Q"], inp["K1"], inp["T"], inp["topk"]
    ref = post_reference(inp)
    p32 = torch.softmax(inp["logits"].view(P * Q, K1), -1)
    s, c = torch.sort(torch.nan_to_num(p32[:, 1:], nan=0.0), dim=-1, descending=True, stable=True)
    ts, tc = s[:, :k].clone(), (c[:, :k] + 1).int()
    ts[ref["nonfinite"]] = math.nan
    tc[ref["nonfinite"]] = torch.arange(1, k + 1, dtype=torch.int32)
    return ts.view(P, Q, k), tc.view(P, Q, k), ref["first"].int().view(P, Q), ref["last"].int().view(P, Q)


def check_postprocess(got, inp, ref, bound):
    """got = (top_score (P, Q, k), top_cat, seg_first (P, Q), seg_last) as ops.postprocess returns them (CPU tensors).  Returns
    the largest score distance; raises AssertionError on: a category outside 1 .. K1-1 or returned twice; scores not in
    descending order, or off the reference's top-k values or the returned category's own probability by more than `bound` of the
    row's largest probability; an exact tie (equal logits, or both probabilities sure to underflow) not broken to the lower
    class; a row without a softmax whose scores are not NaN; a segment other than the reference's."""
    P, Q, K1, k = inp["P"], inp["Q"], inp["K1"], inp["topk"]
    ts, tc, sf, sl = (t.reshape(P * Q, -1) for t in got)
    tc = tc.long()
    assert bool(((tc >= 1) & (tc < K1)).all()), f"category out of 1..{K1 - 1}: {tc[((tc < 1) | (tc >= K1)).any(-1)][:2].tolist()}"
    assert bool((tc.sort(-1).values.diff(dim=-1) > 0).all()), "a category returned twice"
    bad, fin = ref["nonfinite"], ~ref["nonfinite"]
    assert bool(torch.isnan(ts[bad]).all()), "a row without a softmax has a number for a score"
    assert bool(torch.isfinite(ts[fin]).all()), "non-finite score on a finite row"
    worst = 0.0
    if bool(fin.any()):
        s, c = ts[fin].double(), tc[fin]
        probs, lg = ref["probs"][fin], inp["logits"].view(P * Q, K1)[fin].double()
        assert bool((s.diff(dim=-1) <= 0).all()), "scores not in descending order"
        top = probs.amax(-1, keepdim=True)
        worst = max(float(((s - ref["vals"][fin]).abs() / top).max()), float(((s - probs.gather(-1, c)).abs() / top).max()))
        assert worst <= bound, f"scores {worst:.3e} from float64, bound {bound:.3e}"
        # exact ties go to the lower class: a class left out that surely ties with a returned one has the higher index, and
        # two returned classes that surely tie come in ascending order
        low = lg - lg.amax(-1, keepdim=True) < SURE_UNDERFLOW
        mine = lg.gather(-1, c)
        mine_low = low.gather(-1, c)
        taken = torch.zeros_like(low).scatter_(-1, c, True)
        cls = torch.arange(K1)[None, None, :]
        ties = (lg[:, None, :] == mine[:, :, None]) | (low[:, None, :] & mine_low[:, :, None])          # (rows, k, K1)
        skipped = ties & ~taken[:, None, :] & (cls >= 1) & (cls < c[:, :, None])
        assert not bool(skipped.any()), f"tie broken to the higher class (row, slot, class): {skipped.nonzero()[:3].tolist()}"
        pair_tie = (mine[:, 1:] == mine[:, :-1]) | (mine_low[:, 1:] & mine_low[:, :-1])
        assert bool((c[:, 1:] > c[:, :-1])[pair_tie].all()), "tied classes not in ascending order"
    assert torch.equal(sf.flatten().long(), ref["first"]) and torch.equal(sl.flatten().long(), ref["last"]), "segments differ"
    return worst


# ------------------------------------------------------------------------------ post-processing: stand-ins of faults
def _rows_of(inp, kind):
    return [r for r, k in enumerate(inp["lkind"]) if k == kind]


def fault_background_returned(inp):
    ts, tc, sf, sl = post_emulation(inp)
    tc.view(-1, inp["topk"])[_rows_of(inp, "bg_max")[0], 0] = 0
    return ts, tc, sf, sl


def fault_tie_to_higher_class(inp):
    ts, tc, sf, sl = post_emulation(inp)
    k = inp["topk"]
    tc.view(-1, k)[_rows_of(inp, "all_equal")[0]] = torch.arange(inp["K1"] - 1, inp["K1"] - 1 - k, -1, dtype=torch.int32)
    return ts, tc, sf, sl


def fault_segment_includes_valid_len(inp):
    return post_emulation(dict(inp, valid_len=inp["valid_len"] + 1))


def fault_sentinel_category(inp):
    """no candidate beats the initial best: the index keeps its initial value"""
    ts, tc, sf, sl = post_emulation(inp)
    tc.view(-1, inp["topk"])[_rows_of(inp, "all_neg_inf")[0]] = 0x7FFFFFFF
    return ts, tc, sf, sl
