"""GPU: the five depthwise-conv + LayerNorm readers of ONE subject / object stream of backbones.pair_stage, per stream and stage,
over row counts (powers of two from 4 k rows, then the headline's 2048 x 288), in three forms:
  a  today's three vrd_dwconv_ln launches (q / k behind ln1 | v | the other layer's k / v)
  b  two vrd_dwconv_ln_multi launches (q / k / v | the other layer's k / v)
  c  one vrd_dwconv_ln_multi launch of five sets
The forms alternate inside every repetition; the table gives the median time, the bytes a form moves at 2 KiB per row and set, and
the rate of the three-set and five-set launches alone (one read + three / five writes); last column: form c with its five outputs
as column slabs of one buffer (what the bare HBM kernel of LABNOTES.md gains 27 % from: nothing here).  Usage: sos_streams_sweep.py [mode] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from vrdone_amd import ops

mode = sys.argv[1] if len(sys.argv) > 1 else "f16x3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device("cuda:0")
ops.set_precision(mode)
C = 512
g = torch.Generator().manual_seed(5)
names = ("q", "k", "v", "k2", "v2")
sets = {n: dict(weight=(torch.randn(C, 1, 3, generator=g) / 3 ** 0.5).to(dev), gamma=(1 + 0.1 * torch.randn(C, generator=g)).to(dev),
                beta=(0.1 * torch.randn(C, generator=g)).to(dev), pair=True) for n in names}
pre = ((1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev))
shapes = [(r // 256, 256, 256) for r in (1 << e for e in range(12, 20))] + [(2048, 288, 256)]        # (sequences, frames, valid frames)

print(f"# precision {mode}, {reps} repetitions, median ms per stream and stage; GB at 2 KiB per row read or written")
print(f"{'rows':>8} {'a: 3 launches':>14} {'b: 2 launches':>14} {'c: 1 launch':>12} {'b/a':>6} {'c/a':>6}   {'1R+3W TB/s':>10} {'1R+5W TB/s':>10} {'a TB/s':>7} {'c, slabs':>9}")
with torch.no_grad():
    for B, T, valid in shapes:
        rows = B * T
        mask = (torch.arange(T, device=dev)[None, :] < valid).expand(B, T).contiguous()
        x = torch.randn(B, T, C, device=dev) * mask[..., None]
        outs = {n: torch.empty(B, T, C, device=dev) for n in names}
        st = {n: dict(sets[n], out=outs[n]) for n in names}
        nrm = lambda n: dict(st[n], normed=True)          # noqa: E731

        def form_a():
            ops.dwconv_ln(x, [st["q"], st["k"]], mask_out=mask, pre_ln=pre)
            ops.dwconv_ln(x, [st["v"]], mask_out=mask)
            ops.dwconv_ln(x, [st["k2"], st["v2"]], mask_out=mask)

        def own3():
            ops.dwconv_ln_multi(x, [nrm("q"), nrm("k"), st["v"]], mask_out=mask, pre_ln=pre)

        def form_b():
            own3()
            ops.dwconv_ln_multi(x, [st["k2"], st["v2"]], mask_out=mask)

        def form_c():
            ops.dwconv_ln_multi(x, [nrm("q"), nrm("k"), st["v"], st["k2"], st["v2"]], mask_out=mask, pre_ln=pre)

        slab = torch.empty(B, T, 5 * C, device=dev)
        sl = {n: dict(sets[n], out=slab[..., i * C:(i + 1) * C], normed=n in "qk") for i, n in enumerate(names)}

        def form_c_slabs():                                # (the five outputs as column slabs of one buffer)
            ops.dwconv_ln_multi(x, [sl[n] for n in names], mask_out=mask, pre_ln=pre)

        forms = {"a": form_a, "b": form_b, "c": form_c, "own3": own3, "cs": form_c_slabs}
        want = None
        for name in ("a", "b", "c"):                       # (warm-up, and the forms agree bit for bit)
            forms[name]()
            bits = [outs[n].view(torch.int32).clone() for n in names]
            assert want is None or all(torch.equal(p, q) for p, q in zip(bits, want)), name
            want = bits
        times = {k: [] for k in forms}
        for _ in range(reps):
            for name, fn in forms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
        ms = {k: statistics.median(v) for k, v in times.items()}
        tb = lambda passes, t: rows * 2048.0 * passes / (t * 1e-3) / 1e12          # noqa: E731
        print(f"{rows:>8} {ms['a']:>14.4f} {ms['b']:>14.4f} {ms['c']:>12.4f} {ms['b'] / ms['a']:>6.3f} {ms['c'] / ms['a']:>6.3f}   "
              f"{tb(4, ms['own3']):>10.2f} {tb(6, ms['c']):>10.2f} {tb(8, ms['a']):>7.2f} {ms['cs']:>9.4f}", flush=True)
