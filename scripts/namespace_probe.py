"""Namespace data with completeness proofs at the workload's own size (k = 128, 64 namespaces of about 256 shares, each
over three rows): medians over `reps` repetitions after warm-up, the two sides of every comparison in alternating runs.
  open                    cda_square_open
  prove_ns_one            ONE cda_square_prove_namespace call for one namespace over all its rows, into host buffers
  prove_ns_64             ONE call for the 64 namespaces over all their rows
  search_prove_*          the path without it: the rows' leaf namespaces searched on the host (numpy searchsorted over
                          the caller's copy of the shares), then cda_square_prove on the ranges found
  verify_ns_device        cda_nmt_verify_namespace_device on the 64 namespaces' proofs, everything in device memory
  nmt_verify_device       cda_nmt_verify_device on the same inclusion proofs: the NMT leg alone
and the launches alone (HIP events around the kernels, cda_profile_*).  One JSON line.
  python scripts/namespace_probe.py [reps]          (DESIGN.md §18 holds the recorded figures)
  python scripts/namespace_probe.py [reps] open     only the open (runs against any build: CDA_LIB)"""
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
k, w, NS = 128, 256, N.NAMESPACE_SIZE
ctx = cda.Context(0)
ods = bench.gen_ods(k, 0xC0FFEE).copy()
runs = [356] + [256] * 62 + [156]  # runs that start and end mid-row
nss, at = [], 0
for i, n in enumerate(runs):
    ns = bytes(NS - 2) + (2 * i + 2).to_bytes(2, "big")
    ods[at:at + n, :NS] = np.frombuffer(ns, np.uint8)
    nss.append(ns)
    at += n
dev = torch.device("cuda", 0)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def median_ms(f, warm=3):
    for _ in range(warm):
        f()
    ts = sorted(timed(f) for _ in range(reps))
    return round(ts[len(ts) // 2], 3)


def median_alternating(fa, fb, warm=3):
    """Medians of fa and fb, run in turn (drift of the box hits both alike)."""
    for _ in range(warm):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return round(sorted(ta)[reps // 2], 3), round(sorted(tb)[reps // 2], 3)


def kernels_ms(f, *names):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        f()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    return [round(prof.get(n, (0.0, 0))[0] / reps, 4) for n in names]


out = {"k": k, "reps": reps, "build": N.build_info()}
out["open_ms"] = median_ms(lambda: ctx.open_square(ods).close())
if len(sys.argv) > 2 and sys.argv[2] == "open":
    ctx.close()
    print(json.dumps(out))
    sys.exit(0)

from cda import namespace as NSP  # noqa: E402

sq = ctx.open_square(ods)
row_ns = np.ascontiguousarray(ods[:, :NS]).view(f"S{NS}").reshape(k, k)  # the caller's copy: rows of leaf namespaces


def queries_of(names):
    return sq.namespace_queries([(N.AXIS_ROW, r, ns) for ns in names for r in NSP.rows_of_namespace(sq.row_roots, ns)])


def search_prove(names):
    """Without cda_square_prove_namespace: bisect each candidate row's namespaces on the host, prove the ranges."""
    ranges = []
    for ns in names:
        key = np.frombuffer(ns, f"S{NS}")[0]
        for r in NSP.rows_of_namespace(sq.row_roots, ns):
            lo, hi = np.searchsorted(row_ns[r], key, "left"), np.searchsorted(row_ns[r], key, "right")
            if lo < hi:
                ranges.append((N.AXIS_ROW, r, int(lo), int(hi)))
    return sq.prove(ranges)


for label, names in (("one", nss[17:18]), ("64", nss)):
    q = queries_of(names)
    res, _, _, shares = sq.prove_namespace(q)
    out[f"queries_{label}"], out[f"shares_{label}"] = len(q), int(sq.nshares_total)
    assert int(res["nshares"].sum()) == sum(runs[nss.index(x)] for x in names) and (res["kind"] == 1).all()
    assert np.array_equal(shares, search_prove(names)[2])
    # the row selection is part of both paths: timed with the call on both sides
    a, b = median_alternating(lambda: sq.prove_namespace(queries_of(names)), lambda: search_prove(names))
    out[f"prove_ns_{label}_ms"], out[f"search_prove_{label}_ms"] = a, b
    out[f"prove_ns_{label}_kernels_ms"] = kernels_ms(lambda: sq.prove_namespace(q), "square_prove_namespace",
                                                     "namespace_shares")
    out[f"prove_ns_{label}_call_ms"] = median_ms(lambda: sq.prove_namespace(q))
    out[f"prove_ns_{label}_noshares_ms"] = median_ms(lambda: sq.prove_namespace(q, want_shares=False))

# (b) verification on the device: the 64 namespaces' proofs as the prover wrote them, plus absence proofs of the
# namespaces between them for the namespace form alone
q = queries_of(nss)
res, nodes, lhs, shares = sq.prove_namespace(q)
nq, mn, total = len(q), nodes.shape[1], int(sq.nshares_total)
nsd = np.zeros(nq, N.NMT_NS_PROOF_DESC_DTYPE)
for f in ("start", "end", "nnodes"):
    nsd[f] = res[f]
nsd["node_off"] = np.arange(nq, dtype=np.uint32) * mn
nsd["leaf_off"], nsd["nleaves"], nsd["root"], nsd["leaf_hash"] = res["share_off"], res["nshares"], q["index"], \
    N.NO_LEAF_HASH
nmt = np.zeros(nq, N.NMT_PROOF_DESC_DTYPE)
for f in ("start", "end", "node_off", "nnodes", "leaf_off", "root"):
    nmt[f] = nsd[f]
d = {n: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
     for n, a in (("nsd", nsd), ("nmt", nmt), ("ns", q["ns"]), ("roots", sq.row_roots), ("nodes", nodes), ("lhs", lhs),
                  ("shares", shares))}
d_ok = torch.zeros(nq, dtype=torch.uint8, device=dev)
stream = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def verify_ns_device():
    ctx.nmt_verify_namespace_device(nq, d["nsd"].data_ptr(), d["ns"].data_ptr(), d["roots"].data_ptr(), w,
                                    d["nodes"].data_ptr(), nq * mn, d["lhs"].data_ptr(), nq, d["shares"].data_ptr(),
                                    total, d_ok.data_ptr(), stream.cuda_stream)
    stream.synchronize()


def nmt_verify_device():
    ctx.nmt_verify_device(nq, d["nmt"].data_ptr(), d["ns"].data_ptr(), d["roots"].data_ptr(), w, d["nodes"].data_ptr(),
                          nq * mn, d["shares"].data_ptr(), total, d_ok.data_ptr(), stream.cuda_stream)
    stream.synchronize()


verify_ns_device()
assert bool(d_ok.all())
nmt_verify_device()
assert bool(d_ok.all())
out["verify_proofs"], out["verify_leaves"] = nq, total
out["verify_ns_device_ms"], out["nmt_verify_device_ms"] = median_alternating(verify_ns_device, nmt_verify_device)
out["verify_ns_device_kernels_ms"], = kernels_ms(verify_ns_device, "nmt_verify_namespace")
out["nmt_verify_device_kernels_ms"], = kernels_ms(nmt_verify_device, "nmt_verify")
# absence proofs alone: the namespace between every pair, on the rows that hold both neighbours
absent = [bytes(NS - 2) + (2 * i + 3).to_bytes(2, "big") for i in range(len(nss) - 1)]
qa = queries_of(absent)
ra, na_, la, _ = sq.prove_namespace(qa)
assert (ra["kind"] == 2).all()
ad = np.zeros(len(qa), N.NMT_NS_PROOF_DESC_DTYPE)
ad["start"], ad["end"], ad["nnodes"], ad["root"] = ra["start"], ra["end"], ra["nnodes"], qa["index"]
ad["node_off"], ad["leaf_hash"] = np.arange(len(qa), dtype=np.uint32) * mn, np.arange(len(qa), dtype=np.uint32)
out["absence_proofs"] = len(qa)
ok = ctx.nmt_verify_namespace(ad, qa["ns"], sq.row_roots, na_.reshape(-1, N.NODE_SIZE), la, np.zeros((0, 512), np.uint8))
assert ok.all()
out["verify_absence_host_form_ms"] = median_ms(lambda: ctx.nmt_verify_namespace(
    ad, qa["ns"], sq.row_roots, na_.reshape(-1, N.NODE_SIZE), la, np.zeros((0, 512), np.uint8)))
sq.close()
ctx.close()
print(json.dumps(out))
