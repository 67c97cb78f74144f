"""Blob commitment proofs at k = 128 on a block-408-like mix of blobs (one namespace per blob, sizes from one share
to a few thousand, placed by NextShareIndex until the square is full): medians over `reps` repetitions after 3 warm-up
calls, the routes of a comparison run in turn in one process.
  (a) commitments_ms        Square.commitments of all blobs, one call on the retained square
      get_commitment_ms     the route before it: cda_extend_commit_nodes (the row trees exported), then per blob the
                            host walk and cda_merkle_roots -- on the library given as the second argument (the parent
                            commit's build), else on this one; walk_ms is that route without the export
  (b) commitment_proofs_ms / share_proofs_ms and the bytes each returns, for the same ranges
  (c) verify_device_ms      cda_commitment_proofs_verify_device of `nverify` proofs (the mix repeated), and the legs'
                            times by HIP events (cda_profile_*), per call
One JSON line.
  python scripts/commitment_probe.py [reps] [parent libcda.so]       (DESIGN.md §23 holds the recorded figures)"""
import json
import os
import sys
import time

import numpy as np
import torch  # first: libcda then resolves HIP through torch's runtime, as in bench.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
import cda  # noqa: E402
from cda import _native as N  # noqa: E402
from cda import commitment as C  # noqa: E402
from cda import inclusion as I  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
parent = sys.argv[2] if len(sys.argv) > 2 else None
k, threshold, nverify = 128, 64, 4096
ctx = cda.Context(0)
if parent:
    N.lib(parent, older=True)  # an older build lacks the calls this probe is about: bind the ones it has
old = cda.Context(0, lib_path=parent) if parent else ctx
dev = torch.device("cuda", 0)

# the square: blobs back to back, each under a namespace of its own (ascending), the rest tail padding
rng = np.random.default_rng(408)
ods = rng.integers(0, 256, (k * k, 512), dtype=np.uint8)
blobs, cursor, nsid = [], 16, 1
ods[:cursor, :29] = 0
while True:
    n = int(rng.choice([1, 2, 5, 17, 64, 129, 352, 1000, 3000]))
    start = I.next_share_index(cursor, n, threshold)
    if start + n > k * k:
        break
    nsid += 2
    ods[cursor:start, :29] = np.frombuffer(bytes(25) + (nsid - 1).to_bytes(4, "big"), np.uint8)
    ods[start:start + n, :29] = np.frombuffer(bytes(25) + nsid.to_bytes(4, "big"), np.uint8)
    blobs.append((start, n))
    cursor = start + n
ods[cursor:, :29] = np.frombuffer(b"\x00" + b"\xff" * 27 + b"\xfe", np.uint8)  # tail padding
namespaces = [ods[s, :29].tobytes() for s, _ in blobs]
ranges = [(s, s + n) for s, n in blobs]


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


sq = ctx.open_square(ods)
shares = list(ods)
state = {}


def commitments():
    state["new"] = sq.commitments(blobs, threshold)


def get_commitment():
    cacher, dah = I.EDSSubTreeRootCacher.from_shares(shares, old)
    state["cacher"], state["dah"] = cacher, dah
    state["old"] = [I.get_commitment(cacher, dah, s, n, threshold, old) for s, n in blobs]


def walk():
    state["walk"] = [I.get_commitment(state["cacher"], state["dah"], s, n, threshold, old) for s, n in blobs]


def commitment_proofs():
    state["cp"] = sq.commitment_proofs_raw(blobs, threshold)


def share_proofs():
    state["sp"] = sq.share_proofs_raw(ranges)


out = {"k": k, "threshold": threshold, "reps": reps, "blobs": len(blobs), "blob_shares": sum(n for _, n in blobs),
       "build": N.build_info(), "parent_build": N.build_info(parent) if parent else "this library"}
out["commitments_ms"], out["get_commitment_ms"], out["walk_ms"] = median_alternating([commitments, get_commitment, walk])
assert state["new"] == state["old"] == state["walk"]
out["commitment_proofs_ms"], out["share_proofs_ms"] = median_alternating([commitment_proofs, share_proofs])
cp, sp = state["cp"], state["sp"]
assert cp["data_root"] == sp["data_root"] == sq.dah and [x.tobytes() for x in cp["commitments"]] == state["new"]
out["commitment_proof_rows"], out["subtree_roots"] = len(cp["rows"]), len(cp["subtree_roots"])
out["commitment_proofs_bytes"] = int(sum(cp[x].nbytes for x in ("row_off", "rows", "subtree_roots", "row_roots",
                                                                   "leaf_hashes", "aunts", "commitments")) +
                                     int(cp["rows"]["nnodes"].sum()) * N.NODE_SIZE)
out["share_proofs_bytes"] = int(sum(sp[x].nbytes for x in ("row_off", "rows", "row_roots", "leaf_hashes", "aunts",
                                                             "shares")) + int(sp["rows"]["nnodes"].sum()) * N.NODE_SIZE)
out["commitments_kernels_ms"] = kernels_ms(ctx, commitments)
out["commitment_proofs_kernels_ms"] = kernels_ms(ctx, commitment_proofs)

# (c) the mix repeated up to nverify proofs, packed once, verified in device memory
proofs = C.proofs_from_raw(cp, namespaces)
assert all(p.verify_host(sq.dah, c, threshold) == N.CP_VALID for p, c in list(zip(proofs, state["new"]))[:8])
times = -(-nverify // len(proofs))
batch, coms = (proofs * times)[:nverify], (state["new"] * times)[:nverify]
a = C.pack_commitment_proofs(batch, [0] * nverify, list(range(nverify)), [threshold] * nverify)
a["data_roots"] = np.frombuffer(sq.dah, np.uint8).reshape(1, 32)
a["commitments"] = np.frombuffer(b"".join(coms), np.uint8).reshape(-1, 32)
names = ("descs", "rows", "row_roots", "leaf_hashes", "nodes", "subtree_roots", "aunts", "data_roots", "commitments")
d = {x: torch.from_numpy(np.ascontiguousarray(a[x]).view(np.uint8).reshape(-1).copy()).to(dev) for x in names}
d_verdicts = torch.full((nverify,), -1, dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def verify_device():
    ctx.commitment_proofs_verify_device(nverify, d["descs"].data_ptr(), d["rows"].data_ptr(), d["row_roots"].data_ptr(),
                                        d["leaf_hashes"].data_ptr(), len(a["rows"]), d["nodes"].data_ptr(),
                                        len(a["nodes"]), d["subtree_roots"].data_ptr(), len(a["subtree_roots"]),
                                        d["aunts"].data_ptr(), len(a["aunts"]), d["data_roots"].data_ptr(), 1,
                                        d["commitments"].data_ptr(), nverify, d_verdicts.data_ptr(), stream.cuda_stream)
    stream.synchronize()


out["verify_proofs"], out["verify_rows"], out["verify_subtree_roots"] = nverify, len(a["rows"]), len(a["subtree_roots"])
w = [I.sub_tree_width(sum(r.nmt.end - r.nmt.start for r in p.rows), threshold) for p in batch]
spans = [-(-(r.nmt.end - r.nmt.start) // wi) for p, wi in zip(batch, w) for r in p.rows]
out["verify_chain_rows"] = int(sum(1 for x in spans if x == 1))
out["verify_device_ms"], = median_alternating([verify_device])
assert not d_verdicts.cpu().numpy().any()
out["verify_legs_ms"] = kernels_ms(ctx, verify_device)
sq.close()
if old is not ctx:
    old.close()
ctx.close()
print(json.dumps(out))
