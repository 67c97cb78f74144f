"""Bad-encoding fraud proofs at k = 128: medians over `reps` repetitions after 3 warm-up calls, the two sides of every
comparison in alternating runs of one process.
  validate_*              ONE cda_befp_validate call, host buffers: one proof of 128 shares, one of 256, a flood of 64
                          (63 NO_FRAUD, 1 FRAUD; 256 shares each)
  validate_device_*       the same through cda_befp_validate_device, everything in device memory
  composed_*              the same validation from the calls the library had before, once per proof: cda_nmt_verify,
                          cda_rs_decode (when a share is missing), cda_rs_encode, cda_nmt_axis_root, the root compared
                          on the host
  *_kernels_ms            the launches alone (HIP events around the kernels, cda_profile_*), per call
  open_eds / open         cda_square_open_eds against cda_square_open on the same block
One JSON line.
  python scripts/befp_probe.py [reps]          (DESIGN.md §19 holds the recorded figures)"""
import json
import os
import sys
import time

import numpy as np
import torch  # first: libcda then resolves HIP through torch's runtime, as in bench.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
import bench  # noqa: E402
import cda  # noqa: E402
from cda import _native as N  # noqa: E402
from cda import befp, sampling  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
k, w = 128, 256
ctx = cda.Context(0)
ods = bench.gen_ods(k, 0xC0FFEE).copy()
eds = ctx.extend_commit(ods)[0]
bad = eds.copy().reshape(w, w, N.SHARE_SIZE)
ROW_BAD, COL_BAD = k + 3, k + 9
bad[ROW_BAD, COL_BAD, 17] ^= 1  # one Q3 cell
bad = bad.reshape(-1, N.SHARE_SIZE)
dev = torch.device("cuda", 0)
KERNELS = ("befp_prep", "befp_nmt_verify", "befp_gather", "befp_rs_decode", "befp_rs_encode8", "befp_axis_roots",
           "befp_combine")


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def median_ms(f, warm=3):
    for _ in range(warm):
        f()
    ts = sorted(timed(f) for _ in range(reps))
    return round(ts[len(ts) // 2], 3)


def median_alternating(fs, warm=3):
    """Medians of the functions of `fs`, run in turn (drift of the box hits all alike)."""
    for _ in range(warm):
        for f in fs:
            f()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for t, f in zip(ts, fs):
            t.append(timed(f))
    return [round(sorted(t)[reps // 2], 3) for t in ts]


def kernels_ms(f, names):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        f()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {n: round(prof.get(n, (0.0, 0))[0] / reps, 4) for n in names if n in prof}


out = {"k": k, "reps": reps, "build": N.build_info()}
out["open_eds_ms"], out["open_ms"] = median_alternating([lambda: ctx.open_square_eds(eds).close(),
                                                         lambda: ctx.open_square(ods).close()])
out["open_eds_kernels_ms"] = kernels_ms(lambda: ctx.open_square_eds(eds).close(),
                                        ("leaf_hash", "nmt_level1", "nmt_level", "dah"))

sq = ctx.open_square_eds(bad)
roots = [(sq.row_roots, sq.col_roots)]
roots_arr = befp.pack_roots(roots)
fraud128 = befp.create(sq, befp.ROW, ROW_BAD, range(k))          # the bad cell left out: decode, encode, root
fraud256 = befp.create(sq, befp.ROW, ROW_BAD)                     # every share present: the re-encode finds it
flood = [befp.create(sq, befp.ROW, i) for i in range(63)] + [fraud256]
sq.close()


def composition(p):
    """The arrays of one proof for the calls the library had before this one, built outside the timed region."""
    samples = [(1 - p.axis, pos, p.index, share, nmt) for pos, share, nmt in p.shares]
    slots = np.zeros((w, N.SHARE_SIZE), np.uint8)
    present = np.zeros(w, np.uint8)
    for pos, share, _ in p.shares:
        slots[pos] = np.frombuffer(share, np.uint8)
        present[pos] = 1
    committed = bytes(roots[0][p.axis][p.index])
    return p.index, sampling.pack_samples(samples, k), slots, present, committed


def composed(c):
    index, (descs, namespaces, nodes, leaves), slots, present, committed = c
    if not ctx.nmt_verify(descs, namespaces, roots_arr, nodes, leaves).all():
        return befp.BAD_SHARE
    full = slots if present.all() else ctx.rs_decode(slots, present)
    parity = ctx.rs_encode(full[:k])
    try:
        root = ctx.nmt_axis_root(k, index, [full[i].data for i in range(k)] + [parity[i].data for i in range(k)])
    except cda.CdaError as e:
        if e.code != N.E_NS_ORDER:
            raise
        return befp.FRAUD
    return befp.NO_FRAUD if root == committed else befp.FRAUD


for label, proofs in (("one_128", [fraud128]), ("one_256", [fraud256]), ("flood_64", flood)):
    packed = befp.pack(proofs, k)
    want = [befp.NO_FRAUD] * (len(proofs) - 1) + [befp.FRAUD]
    comps = [composition(p) for p in proofs]
    descs, entries, shares, nodes = packed
    d = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
         for a in (descs, entries, shares, nodes, roots_arr)]
    d_ver = torch.zeros(len(proofs), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def fused():
        return ctx.befp_validate(k, *packed, roots_arr)

    def fused_device():
        ctx.befp_validate_device(k, len(proofs), d[0].data_ptr(), d[1].data_ptr(), len(entries), d[2].data_ptr(),
                                 d[3].data_ptr(), len(nodes), d[4].data_ptr(), len(roots_arr), d_ver.data_ptr(),
                                 stream.cuda_stream)
        stream.synchronize()

    def composed_all():
        return [composed(c) for c in comps]

    assert fused().tolist() == want and composed_all() == want
    fused_device()
    assert d_ver.cpu().numpy().tolist() == want
    out[f"proofs_{label}"], out[f"shares_{label}"] = len(proofs), len(entries)
    out[f"validate_{label}_ms"], out[f"validate_device_{label}_ms"], out[f"composed_{label}_ms"] = \
        median_alternating([fused, fused_device, composed_all])
    out[f"validate_{label}_kernels_ms"] = kernels_ms(fused_device, KERNELS)
    out[f"composed_{label}_kernels_ms"] = kernels_ms(composed_all, ("nmt_verify", "axis_rs_decode", "axis_rs_encode8",
                                                                     "axis_roots"))
ctx.close()
print(json.dumps(out))
