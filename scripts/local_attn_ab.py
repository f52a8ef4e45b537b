#!/usr/bin/env python3
"""Do two builds of the library compute the same bits in the banded attention and the pair-row flash attention?

    python scripts/local_attn_ab.py --a /path/to/parent/libvrdone_hip.so --out profiles/local_attn_ab.json      # on the GPU box

Every run is a child process under `timeout -k 10` that loads ONE library (VRDONE_HIP_LIB: --a, then this tree's) and prints the
sha256 digest of every output; the first child that fails ends the visit (nothing more is started on the device).  The kernels
have no atomics, so all digests must be equal; exit status 1 if one is not.

  local      every (width, heads, window, rel_pe) of tests/local_heads_cases.py (ALL_OP_CASES) and the two shipped head counts at
             width 512: vrd_local_attn to f32 rows and to both pair formats, vrd_local_attn_segs over a two-group table,
             vrd_local_attn_drop at p = 0.1 with a pinned seed, vrd_local_attn_bwd and vrd_local_attn_drop_bwd with their
             scratch halves P and dS
  local_row  the forward again under VRD_LOCAL_STRIP=0 (the per-row kernel; the switch is read once per process)
  flash      vrd_attention_pair and vrd_attention_pair_segs at 4 x 128, 8 x 64 and 16 x 32 heads, Tq = Tk of 33 and 160 (from 160
             on head_dim 128 takes the 64-queries-per-wave kernel), both pair formats, products = 1 where it exists, and a
             two-group table with a group on each kernel
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CHILDREN = {"local": {}, "local_row": {"VRD_LOCAL_STRIP": "0"}, "flash": {}}


def digest(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def child_local(forward_only):
    import ctypes
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    import local_heads_cases as LH
    from vrdone_amd import _hip
    lib, dev, out = _hip.lib, torch.device("cuda"), {}
    seed = torch.tensor([0x5EED5EED1234], dtype=torch.int64, device=dev)
    cases = LH.ALL_OP_CASES + [(512, H, W, rel) for H in (4, 8) for W in LH.WINDOWS for rel in (False, True)]
    for C, H, W, rel in cases:
        q, k, v, dO, rel_pe = LH.core_inputs(C, H, W, rel)
        B, T = LH.B, LH.seq_len(W)
        rows = lambda x: x.transpose(1, 2).contiguous().reshape(B * T, C).to(dev)      # (B, C, T) -> channels-last rows
        q, k, v, dO = rows(q), rows(k), rows(v), rows(dO)
        mask = LH.mask(W).reshape(B * T).to(torch.uint8).to(dev)
        rp = rel_pe.reshape(H, W).contiguous().to(dev) if rel else None
        rpp = rp.data_ptr() if rel else None
        tag, hw = LH.tag(C, H, W, rel), W // 2
        new = lambda *shape: torch.full(shape, float("nan"), device=dev)

        def call(name, *args):
            rc = getattr(lib, name)(*args)
            assert rc == 0, (name, tag, rc, lib.vrd_last_error().decode())

        for fmt in (_hip.PAIR_NONE, _hip.PAIR_BF16, _hip.PAIR_F16):
            o = new(B * T, C)
            call("vrd_local_attn", q.data_ptr(), k.data_ptr(), v.data_ptr(), C, mask.data_ptr(), rpp, B, T, C, H, hw, o.data_ptr(), C, fmt, None)
            out[f"{tag}/fwd/pair{fmt}"] = digest(o)
        if forward_only:
            continue
        # the same rows as one sequence of T frames and 2 (B - 1) of T / 2 (T is even)
        table = _hip.RowSegs.of([(0, 1, T), (T, 2 * (B - 1), T // 2)])
        o = new(B * T, C)
        call("vrd_local_attn_segs", q.data_ptr(), k.data_ptr(), v.data_ptr(), C, mask.data_ptr(), rpp, ctypes.byref(table), C, H, hw,
             o.data_ptr(), C, _hip.PAIR_NONE, None)
        out[f"{tag}/fwd/segs"] = digest(o)
        o = new(B * T, C)
        call("vrd_local_attn_drop", q.data_ptr(), k.data_ptr(), v.data_ptr(), C, mask.data_ptr(), rpp, B, T, C, H, hw, seed.data_ptr(), 7, 64, 0.1,
             o.data_ptr(), C, None)
        out[f"{tag}/drop_fwd"] = digest(o)
        for name, extra in (("vrd_local_attn_bwd", ()), ("vrd_local_attn_drop_bwd", (seed.data_ptr(), 7, 64, 0.1))):
            dq, dk, dv, scratch = new(B * T, C), new(B * T, C), new(B * T, C), new(2, B * T * H * W)
            call(name, q.data_ptr(), k.data_ptr(), v.data_ptr(), C, dO.data_ptr(), C, mask.data_ptr(), rpp, B, T, C, H, hw, *extra,
                 dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), C, scratch.data_ptr(), None)
            for what, t in (("dq", dq), ("dk", dk), ("dv", dv), ("P", scratch[0]), ("dS", scratch[1])):
                out[f"{tag}/{name[4:]}/{what}"] = digest(t)
    return out


def pair_rows(x, f16):
    """(rows, W) f32 -> pair rows: per block of 32 channels 32 hi halves, then 32 lo halves (csrc/vrd_common.h)"""
    import torch
    y = x * 16.0 if f16 else x
    dt = torch.float16 if f16 else torch.bfloat16
    hi = y.to(dt)
    lo = (y - hi.float()).to(dt)
    r, w = x.shape
    both = torch.cat([hi.view(torch.int16).reshape(r, w // 32, 32), lo.view(torch.int16).reshape(r, w // 32, 32)], dim=2)
    return both.reshape(r, 2 * w).contiguous().view(torch.float32)


def child_flash():
    import ctypes
    import torch
    sys.path.insert(0, REPO)
    from vrdone_amd import _hip
    lib, dev, out = _hip.lib, torch.device("cuda"), {}
    B = 3
    for H, hd in ((4, 128), (8, 64), (16, 32)):
        C = H * hd
        for f16 in (False, True):
            fmt = _hip.PAIR_F16 if f16 else _hip.PAIR_BF16
            for products in ((0, 1) if f16 and hd != 32 else (0,)):
                for T in (33, 160):
                    g = torch.Generator().manual_seed(7000 + 10 * hd + T + int(f16))
                    q, k, v = (pair_rows(torch.randn(B * T, C, generator=g), f16).to(dev) for _ in range(3))
                    kv_mask = (torch.arange(T)[None] < torch.tensor([T, T - 5, 1])[:, None]).reshape(B * T).to(torch.uint8).to(dev)
                    for out_pair in (_hip.PAIR_NONE, fmt):
                        o = torch.full((B * T, C), float("nan"), device=dev)
                        rc = lib.vrd_attention_pair(q.data_ptr(), C, k.data_ptr(), v.data_ptr(), C, kv_mask.data_ptr(), kv_mask.data_ptr(), B, T, T, H,
                                                    hd, o.data_ptr(), C, out_pair, fmt, None, products)
                        assert rc == 0, (H, hd, f16, products, T, rc, lib.vrd_last_error().decode())
                        out[f"pair/h{H}x{hd}/fmt{fmt}/p{products}/T{T}/out{out_pair}"] = digest(o)
                # two groups in one row space: 2 sequences of 33 rows, then 1 of 160 (at head_dim 128 a group on each kernel)
                R = 2 * 33 + 160
                g = torch.Generator().manual_seed(7500 + 10 * hd + int(f16))
                q, k, v = (pair_rows(torch.randn(R, C, generator=g), f16).to(dev) for _ in range(3))
                valid = torch.cat([torch.arange(33) < 33, torch.arange(33) < 20, torch.arange(160) < 150]).to(torch.uint8).to(dev)
                table = _hip.RowSegs.of([(0, 2, 33), (66, 1, 160)])
                o = torch.full((R, C), float("nan"), device=dev)
                rc = lib.vrd_attention_pair_segs(q.data_ptr(), C, k.data_ptr(), v.data_ptr(), C, valid.data_ptr(), valid.data_ptr(), ctypes.byref(table),
                                                 ctypes.byref(table), H, hd, o.data_ptr(), C, fmt, fmt, None, products)
                assert rc == 0, (H, hd, f16, products, rc, lib.vrd_last_error().decode())
                out[f"pair_segs/h{H}x{hd}/fmt{fmt}/p{products}"] = digest(o)
    return out


def run_child(kind, lib_path, limit):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("VRD_FLASH_", "VRD_LOCAL_"))}
    env.update(CHILDREN[kind], VRDONE_HIP_LIB=lib_path)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind]
    res = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if res.returncode != 0:                    # a failed run ends the visit: nothing more is started on the device
        sys.exit(f"{kind} with {lib_path} failed ({res.returncode}):\n{res.stderr[-3000:]}")
    return json.loads(res.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(CHILDREN))
    ap.add_argument("--a", help="the library to compare with (the parent commit's build)")
    ap.add_argument("--b", default=os.path.join(REPO, "vrdone_amd", "csrc", "libvrdone_hip.so"))
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child_flash() if args.child == "flash" else child_local(args.child == "local_row")))
        sys.exit(0)
    result, unequal = {"runs": {}}, 0
    for kind in CHILDREN:
        da = run_child(kind, os.path.abspath(args.a), args.limit)
        db = run_child(kind, os.path.abspath(args.b), args.limit)
        diff = sorted(key for key in set(da) | set(db) if da.get(key) != db.get(key))
        unequal += len(diff)
        all_digests = hashlib.sha256(json.dumps(sorted(db.items())).encode()).hexdigest()[:16]
        result["runs"][kind] = {"outputs": len(db), "unequal": diff, "digest_of_digests": all_digests}
        print(kind, json.dumps(result["runs"][kind]), flush=True)
    result["unequal"] = unequal
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    sys.exit(1 if unequal else 0)
