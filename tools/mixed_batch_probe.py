#!/usr/bin/env python3
"""Times the mixed-size batch (cda_extend_commit_mixed_device) against the parent commit's best form, and the
one-workgroup kernel against the grouped route at each small size.  Not bench.py; needs a GPU.

Part 1, the mix: 512 blocks shuffled with a fixed seed, 128 / 128 / 96 / 96 / 32 / 16 / 12 / 4 of k = 1 / 2 / 4 / 8 / 16
/ 32 / 64 / 128.  This is a stand-in: the repository holds no chain statistics.
  baseline  a libcda.so built from the parent commit (--parent PATH), given the form that favours it most: the blocks
            pre-sorted by k in HBM and one cda_extend_commit_device per size (8 calls);
  mixed     one cda_extend_commit_mixed_device over the shuffled blocks in HBM;
  mixed_sorted        the same call over the baseline's sorted buffers (what the header advises a caller who wants
                      its large blocks batched);
  mixed_small_max_0   the shuffled call with the fused kernel off.
Part 2, small sizes alone: n = 1, 16, 128, 1024 blocks of one k in {1, 2, 4, 8}, through the mixed call with
CDA_OPT_MIXED_SMALL_MAX = 8 (fused) and = 0 (grouped: the block pipeline on the n blocks).

Every shape is warmed up, the two arms alternate within one call of this tool, and each timed region ends in a
synchronise.  One JSON line per result; repeat the command to see the run-to-run spread."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

COUNTS = {1: 128, 2: 128, 4: 96, 8: 96, 16: 32, 32: 16, 64: 12, 128: 4}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="libcda.so built from the parent commit (part 1's baseline; part 1 is skipped without)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-small", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mixed_batch_probe: no GPU")
    torch.cuda.init()
    import cda
    from cda import _native as N
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def buffers(ks):
        off = N.mixed_offsets(ks)
        g = torch.Generator(device=dev)
        g.manual_seed(len(ks))
        ods = torch.randint(0, 256, (int(off["ods"][-1]),), dtype=torch.uint8, device=dev, generator=g)
        return (off, ods, torch.empty((int(off["eds"][-1]),), dtype=torch.uint8, device=dev),
                torch.empty((int(off["recs"][-1]) * 96,), dtype=torch.uint8, device=dev),
                torch.empty((len(ks) * 32,), dtype=torch.uint8, device=dev),
                torch.empty((len(ks),), dtype=torch.int64, device=dev))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(arms):
        """{name: [ms]}: every arm warmed up, then the arms in turn, reps times."""
        for fn in arms.values():
            for _ in range(args.warmup):
                timed(fn)
        out = {name: [] for name in arms}
        for _ in range(args.reps):
            for name, fn in arms.items():
                out[name].append(timed(fn))
        return out

    def report(what, times, **extra):
        row = dict(what=what, **extra)
        for name, t in times.items():
            row[name] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4),
                             p90_ms=round(sorted(t)[int(0.9 * (len(t) - 1))], 4))
        print(json.dumps(row), flush=True)
        return row

    ctx = cda.Context(0)
    print(json.dumps(dict(what="build", new=N.build_info(), reps=args.reps, warmup=args.warmup,
                          device=torch.cuda.get_device_name(0))), flush=True)

    # ---- part 1: the mix ----
    if args.parent:
        N.lib(args.parent, older=True)
        pctx = cda.Context(0, lib_path=args.parent)
        rng = np.random.default_rng(20260)
        ks = np.repeat(list(COUNTS), list(COUNTS.values()))
        rng.shuffle(ks)
        ks = [int(k) for k in ks]
        off, ods, eds, roots, dah, status = buffers(ks)
        # the baseline's buffers: the same blocks sorted by k, one contiguous range per size
        s_off, s_ods, s_eds, s_roots, s_dah, s_status = buffers(sorted(ks))
        sizes, b0 = [], 0
        for k, n in COUNTS.items():
            sizes.append((k, n, b0))
            b0 += n

        def baseline():
            for k, n, b in sizes:
                pctx.extend_commit_device(k, n, s_ods.data_ptr() + int(s_off["ods"][b]),
                                          s_eds.data_ptr() + int(s_off["eds"][b]),
                                          s_roots.data_ptr() + int(s_off["recs"][b]) * 96, s_dah.data_ptr() + 32 * b,
                                          s_status.data_ptr() + 8 * b, stream.cuda_stream)

        def mixed():
            ctx.extend_commit_mixed_device(ks, ods.data_ptr(), eds.data_ptr(), roots.data_ptr(), dah.data_ptr(),
                                           status.data_ptr(), stream.cuda_stream)

        def grouped_small():  # the new call with the fused kernel off: what the routing alone costs
            ctx.set_option(N.OPT_MIXED_SMALL_MAX, 0)
            mixed()
            ctx.set_option(N.OPT_MIXED_SMALL_MAX, default_small)

        sorted_ks = sorted(ks)

        def mixed_sorted():  # the caller has ordered its blocks by size: one fused launch and one run per large size
            ctx.extend_commit_mixed_device(sorted_ks, s_ods.data_ptr(), s_eds.data_ptr(), s_roots.data_ptr(),
                                           s_dah.data_ptr(), s_status.data_ptr(), stream.cuda_stream)

        default_small = 8
        runs = sum(1 for i, k in enumerate(ks) if k > 8 and (i == 0 or ks[i - 1] != k))
        for small_max in (8, 4, 2):
            default_small = small_max
            ctx.set_option(N.OPT_MIXED_SMALL_MAX, small_max)
            report("mix", alternate(dict(parent_sorted_per_size=baseline, mixed=mixed, mixed_sorted=mixed_sorted,
                                         mixed_small_max_0=grouped_small)),
                   blocks=len(ks), small_max=small_max, runs_above_8_shuffled=runs)
        ctx.set_option(N.OPT_MIXED_SMALL_MAX, 8)
        pctx.close()

    # ---- part 2: small sizes alone ----
    if not args.skip_small:
        for k in (1, 2, 4, 8):
            for n in (1, 16, 128, 1024):
                ks = [k] * n
                off, ods, eds, roots, dah, status = buffers(ks)

                def call(small_max):
                    def fn():
                        ctx.set_option(N.OPT_MIXED_SMALL_MAX, small_max)
                        ctx.extend_commit_mixed_device(ks, ods.data_ptr(), eds.data_ptr(), roots.data_ptr(),
                                                       dah.data_ptr(), status.data_ptr(), stream.cuda_stream)
                    return fn
                t = alternate(dict(fused=call(8), grouped=call(0)))
                report("small", t, k=k, blocks=n,
                       fused_not_slower=statistics.median(t["fused"]) <= statistics.median(t["grouped"]))
        ctx.set_option(N.OPT_MIXED_SMALL_MAX, 8)
    ctx.close()


if __name__ == "__main__":
    main()
