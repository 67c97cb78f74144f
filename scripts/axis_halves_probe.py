"""Halves of rows and columns at k = 128: medians over `reps` repetitions after 3 warm-up calls, the routes of a
comparison run in turn in one process.
  (a) verify_host_ms      ONE cda_axis_halves_verify call over 256 halves from host buffers: the 128 ODS rows as first
                          sides and the 128 bottom rows as second sides
      verify_device_ms    cda_axis_halves_verify_device on the same halves already in device memory (with the wait)
      verify_kernels_ms   the launches alone (HIP events around the kernels, cda_profile_*), per call
  (b) per_axis_ms         the same 256 axes by the calls the library had before: cda_rs_encode or cda_rs_decode, then
                          cda_nmt_axis_root, one axis per call through host buffers
  (c) rebuild_axes_ms     cda_square_rebuild_axes from the 128 first-side ODS rows
      rebuild_samples_ms  cda_square_rebuild from the same cells as 16,384 proved samples (DESIGN §22's route)
      open_ms             cda_square_open of the ODS: the floor when every ODS row is known and trusted
One JSON line, also written to profiles/axis_halves_probe.json.
  python scripts/axis_halves_probe.py [reps]                         (DESIGN.md §26 holds the recorded figures)"""
import ctypes
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
k, w = 128, 256
ctx = cda.Context(0)
dev = torch.device("cuda", 0)
ods = bench.gen_ods(k, 0xC0FFEE).copy()
eds, rr, cr, dah = ctx.extend_commit(ods)
grid = eds.reshape(w, w, N.SHARE_SIZE)
roots = np.concatenate([rr, cr])

# (a): rows 0 .. k-1 as first sides, rows k .. 2k-1 as second sides
descs = np.zeros(w, N.AXIS_HALF_DESC_DTYPE)
descs["index"] = np.arange(w)
descs["side"] = (np.arange(w) >= k).astype(np.uint32)
shares = np.ascontiguousarray(np.stack([grid[i, (k if i >= k else 0):(w if i >= k else k)] for i in range(w)]))
want = np.zeros(w, np.uint8)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


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


def kernels_ms(f):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        f()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return {name: round(ms / reps, 4) for name, (ms, _) in sorted(prof.items())}


def verify_host():
    assert np.array_equal(ctx.axis_halves_verify(k, descs, shares, roots), want)


d = {name: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
     for name, a in (("descs", descs), ("shares", shares), ("roots", roots))}
d_statuses = torch.empty(w, dtype=torch.uint8, device=dev)
stream = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def verify_device():
    ctx.axis_halves_verify_device(k, w, d["descs"].data_ptr(), d["shares"].data_ptr(), d["roots"].data_ptr(),
                                  len(roots), d_statuses.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()


# (b): one axis per call
L = ctx._L
axis = np.zeros((w, N.SHARE_SIZE), np.uint8)
present = np.zeros(w, np.uint8)
root = np.empty(N.NODE_SIZE, np.uint8)
err = N.ErrInfo()


def per_axis():
    for i in range(w):
        if i < k:
            axis[:k] = shares[i]
            rc = L.cda_rs_encode(ctx._h, k, N.SHARE_SIZE, N._p(axis[:k]), N._p(axis[k:]))
        else:
            axis[k:] = shares[i]
            present[:k], present[k:] = 0, 1
            rc = L.cda_rs_decode(ctx._h, k, N.SHARE_SIZE, N._p(axis), N._p(present))
        assert rc == N.OK
        rc = L.cda_nmt_axis_root(ctx._h, k, i, w, N.SHARE_SIZE, N._p(axis), N._p(root), ctypes.byref(err))
        assert rc == N.OK and root.tobytes() == rr[i].tobytes()


# (c)
first = descs[:k]
first_shares = np.ascontiguousarray(shares[:k])


def rebuild_axes():
    rc, sq, statuses, _, _, _ = ctx.square_rebuild_axes(first, first_shares, rr, cr)
    assert rc == N.OK and sq.dah == dah
    sq.close()


nq, mn = k * k, 8
q = np.zeros(nq, N.RANGE_QUERY_DTYPE)
q["index"], q["start"] = np.divmod(np.arange(nq, dtype=np.uint32), k)
q["end"] = q["start"] + 1
with ctx.open_square(ods) as src:
    counts, s_nodes, s_shares = src.prove(q)
assert (counts == mn).all()
s_nodes = np.ascontiguousarray(s_nodes[:, :mn]).reshape(-1, N.NODE_SIZE)
s_descs = np.zeros(nq, N.SAMPLE_DESC_DTYPE)
s_descs["index"], s_descs["pos"] = q["index"], q["start"]
s_descs["node_off"], s_descs["nnodes"] = np.arange(nq, dtype=np.uint32) * mn, mn


def rebuild_samples():
    rc, sq, _, _, _, _ = ctx.rebuild_square_status(s_descs, s_shares, s_nodes, rr, cr)
    assert rc == N.OK and sq.dah == dah
    sq.close()


def open_ods():
    sq = ctx.open_square(ods)
    assert sq.dah == dah
    sq.close()


verify_device()
assert np.array_equal(d_statuses.cpu().numpy(), want)
out = {"k": k, "reps": reps, "halves": w, "build": N.build_info()}
out["verify_host_ms"], out["verify_device_ms"], out["per_axis_ms"] = median_alternating(
    [verify_host, verify_device, per_axis])
out["rebuild_axes_ms"], out["rebuild_samples_ms"], out["open_ms"] = median_alternating(
    [rebuild_axes, rebuild_samples, open_ods])
out["verify_kernels_ms"] = kernels_ms(verify_device)
out["rebuild_axes_kernels_ms"] = kernels_ms(rebuild_axes)
out["ratios"] = {"verify_host/per_axis": round(out["verify_host_ms"] / out["per_axis_ms"], 4),
                 "verify_device/per_axis": round(out["verify_device_ms"] / out["per_axis_ms"], 4),
                 "rebuild_axes/rebuild_samples": round(out["rebuild_axes_ms"] / out["rebuild_samples_ms"], 4),
                 "rebuild_axes/open": round(out["rebuild_axes_ms"] / out["open_ms"], 4)}
ctx.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "axis_halves_probe.json"), "w") as f:
    f.write(line + "\n")
print(line)
