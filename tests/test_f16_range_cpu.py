"""The operand range of the VRD_PAIR_F16 format, without a GPU: the format's own model (torch.float16 planes of x * 2^4) against
the rule the kernels' RangeTrack applies (|x * 2^4| >= 65520 reports), and the host's table of the flag word's bits against the
enum the kernels use.  The GPU side is tests/test_gpu_f16_range.py."""
import os
import re
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f16x1_emulation import ACT_EXP  # noqa: E402

SCALE = 2.0 ** ACT_EXP
LIMIT = 65520.0           # RangeTrack::report (vrd_common.h): amax >= 65520 sets the tag


def planes(x):
    """hi / lo f16 planes of float32 values, formed like split_n<true>: y = x * 2^4 in f32, hi = f16(y), lo = f16(y - hi)"""
    y = x.float() * SCALE
    hi = y.to(torch.float16)
    lo = (y - hi.float()).to(torch.float16)
    return y, hi, lo


def f32(v):
    return torch.tensor([v], dtype=torch.float64).float()


def neighbours(v):
    t = f32(v)
    return [torch.nextafter(t, f32(0.0)), t, torch.nextafter(t, f32(float("inf")) * torch.sign(t))]


CASES = [4094.0, None, 4095.0, -4095.0, 65519.0 / 16, 65520.0 / 16]          # None: nextafter(4095, 0)


@pytest.mark.parametrize("value", CASES)
def test_kernel_rule_agrees_with_the_format_at_the_threshold(value):
    """`finite(hi) and finite(lo)` of the float16 model against the kernels' `|x * 16| >= 65520` rule, at the value and at both of
    its float32 neighbours."""
    xs = [torch.nextafter(f32(4095.0), f32(0.0))] if value is None else neighbours(value)
    for x in xs:
        y, hi, lo = planes(x)
        fits = bool(torch.isfinite(hi).all() and torch.isfinite(lo).all())
        reported = bool(y.abs() >= LIMIT)
        assert fits == (not reported), (float(x), float(y), float(hi), float(lo))


def test_threshold_values_of_the_gpu_tests():
    """What tests/test_gpu_f16_range.py relies on: 4095 does not fit (hi = inf, lo = -inf), 4094 decodes exactly, and the last
    float32 below 4095 still fits as hi = 65504, lo = 16 (15.996 rounded)."""
    y, hi, lo = planes(f32(4095.0))
    assert float(y) == 65520.0 and float(hi) == float("inf") and float(lo) == float("-inf")
    y, hi, lo = planes(f32(4094.0))
    assert float(hi) == 65504.0 and float(lo) == 0.0 and (hi.float() + lo.float()) / SCALE == 4094.0
    y, hi, lo = planes(torch.nextafter(f32(4095.0), f32(0.0)))
    assert float(hi) == 65504.0 and float(lo) == 16.0 and bool(torch.isfinite(lo))
    for big in (8192.0, -8192.0):
        assert not bool(torch.isfinite(planes(f32(big))[1]))
    for small in (2048.0, -2048.0):
        y, hi, lo = planes(f32(small))
        assert float(hi.float() + lo.float()) == float(y)


def test_decode_error_bound():
    """|y - hi - lo| <= 2^-22 |y| for 1,000 seeded values x in [2^-2, 4094] (both signs), y = 16 x: hi rounds to 2^-11 |y|, lo to
    2^-11 of that residual or, where lo is an f16 subnormal, to 2^-25 absolute, which is below 2^-22 |y| from |y| = 4 on."""
    g = torch.Generator().manual_seed(4094)
    mag = torch.exp2(torch.rand(1000, generator=g, dtype=torch.float64) * (torch.log2(torch.tensor(4094.0, dtype=torch.float64)) + 2.0) - 2.0)
    x = (mag.clamp(0.25, 4094.0) * torch.where(torch.rand(1000, generator=g) < 0.5, -1.0, 1.0).double()).float()
    y, hi, lo = planes(x)
    assert bool(torch.isfinite(hi).all() and torch.isfinite(lo).all())
    err = (y.double() - hi.double() - lo.double()).abs()
    assert bool((err <= 2.0 ** -22 * y.double().abs()).all()), float((err / y.double().abs()).max())


def _enum_bits():
    src = open(os.path.join(REPO, "vrdone_amd", "csrc", "vrd_common.h")).read()
    body = re.search(r"enum RangeTag : unsigned \{(.*?)\};", src, re.S).group(1)
    return {name: int(val) for name, val in re.findall(r"(RANGE_\w+)\s*=\s*(\d+)u", body)}


def test_range_tags_match_the_enum():
    from vrdone_amd import _hip, ops
    bits = _enum_bits()
    assert len(bits) == 7 and sorted(bits.values()) == [1, 2, 4, 8, 16, 32, 64]
    assert sorted(_hip.RANGE_TAGS) == sorted(bits.values())
    names = [_hip.RANGE_TAGS[b] for b in sorted(_hip.RANGE_TAGS)]
    assert len(set(names)) == len(names) and all(names)
    for b, name in _hip.RANGE_TAGS.items():
        assert ops.describe_range(b) == name
    assert ops.describe_range(0) == "none"
    assert ops.describe_range(2 | 32) == f"{_hip.RANGE_TAGS[2]}, {_hip.RANGE_TAGS[32]}"
    # every reporting entry point is named in the table of its tag
    for bit, kernels in {1: ("bct_to_btc", "pack_pairs", "gather_pairs"), 2: ("layernorm", "conv_ln"), 4: ("dwconv_ln",), 8: ("gemm",),
                         16: ("gemm", "attention_rows", "attention_bwd"), 32: ("local_attn", "attention")}.items():
        for kname in kernels:
            assert kname in _hip.RANGE_TAGS[bit], (bit, kname)
