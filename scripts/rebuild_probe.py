"""A square rebuilt from proved samples at k = 128, a fixed-seed 50 % of the cells proved on the row axis: medians over
`reps` repetitions after 3 warm-up calls, the routes run in turn in one process.
  rebuild_ms          ONE cda_square_rebuild call from host buffers (samples up, nothing else crosses the bus)
  device_chain_ms     the samples already in device memory: cda_samples_assemble_device, the presence map back,
                      cda_repair_device, cda_square_open_eds_device
  composed_ms         the same job through the calls the library had before: cda_nmt_verify, a numpy scatter of the
                      accepted cells into a host square, cda_repair, cda_square_open_eds -- on the library given as
                      the second argument (the parent commit's build), else on this one
  *_kernels_ms        the launches alone (HIP events around the kernels, cda_profile_*), per call
One JSON line.
  python scripts/rebuild_probe.py [reps] [parent libcda.so]          (DESIGN.md §22 holds the recorded figures)"""
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
parent = sys.argv[2] if len(sys.argv) > 2 else None
k, w = 128, 256
nq, mn = w * w, 8
ctx = cda.Context(0)
if parent:
    # an older build lacks the calls this probe is about, which cda.lib() rightly refuses: bind the ones it has
    older, this = ctypes.CDLL(parent), N.lib()
    for name in N.EXPORTS:
        if hasattr(older, name):
            getattr(older, name).restype = getattr(this, name).restype
            getattr(older, name).argtypes = getattr(this, name).argtypes
    N._libs[parent] = older
old = cda.Context(0, lib_path=parent) if parent else ctx
dev = torch.device("cuda", 0)
ods = bench.gen_ods(k, 0xC0FFEE).copy()

q = np.zeros(nq, N.RANGE_QUERY_DTYPE)
q["index"], q["start"] = np.divmod(np.arange(nq, dtype=np.uint32), w)
q["end"] = q["start"] + 1
with ctx.open_square(ods) as src:
    counts, all_nodes, all_shares = src.prove(q)
    rr, cr, dah = src.row_roots.copy(), src.col_roots.copy(), src.dah
assert (counts == mn).all()
pick = np.flatnonzero(np.random.default_rng(128).random(nq) < 0.5)
n = len(pick)
shares = np.ascontiguousarray(all_shares[pick])
nodes = np.ascontiguousarray(all_nodes[pick][:, :mn]).reshape(-1, N.NODE_SIZE)
descs = np.zeros(n, N.SAMPLE_DESC_DTYPE)
descs["index"], descs["pos"] = q["index"][pick], q["start"][pick]
descs["node_off"], descs["nnodes"] = np.arange(n, dtype=np.uint32) * mn, mn
roots = np.concatenate([rr, cr])
# the older calls' form of the same samples
vdescs = np.zeros(n, N.NMT_PROOF_DESC_DTYPE)
vdescs["start"], vdescs["end"] = descs["pos"], descs["pos"] + 1
vdescs["node_off"], vdescs["nnodes"], vdescs["leaf_off"] = descs["node_off"], mn, np.arange(n, dtype=np.uint32)
vdescs["root"] = descs["index"]
ns = np.full((n, N.NAMESPACE_SIZE), 0xFF, np.uint8)
q0 = (descs["index"] < k) & (descs["pos"] < k)
ns[q0] = shares[q0, :N.NAMESPACE_SIZE]


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


def kernels_ms(c, f):
    c.profile_enable(True)
    c.profile_reset()
    for _ in range(reps):
        f()
    prof = c.profile_read()
    c.profile_enable(False)
    return {name: round(ms / reps, 4) for name, (ms, _) in sorted(prof.items())}


def rebuild():
    rc, sq, statuses, present, _, _ = ctx.rebuild_square_status(descs, shares, nodes, rr, cr)
    assert rc == N.OK and sq.dah == dah
    sq.close()


d = {name: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
     for name, a in (("descs", descs), ("shares", shares), ("nodes", nodes), ("roots", roots))}
d_eds = torch.empty(nq * N.SHARE_SIZE, dtype=torch.uint8, device=dev)
d_present = torch.empty(nq, dtype=torch.uint8, device=dev)
d_statuses = torch.empty(n, dtype=torch.uint8, device=dev)
stream = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def device_chain():
    ctx.samples_assemble_device(k, n, d["descs"].data_ptr(), d["shares"].data_ptr(), d["nodes"].data_ptr(),
                                len(nodes), d["roots"].data_ptr(), d_eds.data_ptr(), d_present.data_ptr(),
                                d_statuses.data_ptr(), stream.cuda_stream)
    with torch.cuda.stream(stream):
        present = d_present.cpu().numpy()
    rc, present, _ = ctx.repair_device(k, d_eds.data_ptr(), present, rr, cr, stream.cuda_stream)
    assert rc == N.OK
    sq = ctx.open_square_eds_device(k, d_eds.data_ptr(), stream.cuda_stream)
    assert sq.dah == dah
    sq.close()


cells = (descs["index"].astype(np.int64) * w + descs["pos"])
host_eds = np.zeros((nq, N.SHARE_SIZE), np.uint8)
host_present = np.zeros(nq, np.uint8)


def composed():
    ok = old.nmt_verify(vdescs, ns, roots, nodes, shares).astype(bool)
    host_eds[:] = 0
    host_present[:] = 0
    host_eds[cells[ok]] = shares[ok]
    host_present[cells[ok]] = 1
    rc, _, _, _ = old.repair_status(host_eds, host_present, rr, cr, inplace=True)
    assert rc == N.OK
    sq = old.open_square_eds(host_eds)
    assert sq.dah == dah
    sq.close()


out = {"k": k, "reps": reps, "samples": int(n), "build": N.build_info(),
       "composed_build": N.build_info(parent) if parent else "this library"}
out["rebuild_ms"], out["device_chain_ms"], out["composed_ms"] = median_alternating([rebuild, device_chain, composed])
out["rebuild_kernels_ms"] = kernels_ms(ctx, rebuild)
out["device_chain_kernels_ms"] = kernels_ms(ctx, device_chain)
out["composed_kernels_ms"] = kernels_ms(old, composed)
if old is not ctx:
    old.close()
ctx.close()
print(json.dumps(out))
