"""Sample proofs at the workload's own size (k = 128): medians over `reps` repetitions after warm-up of
  open            cda_square_open (extend + commit + every tree node retained)
  prove           cda_square_prove of all 65,536 single-cell row queries, with and without the cells, into host buffers
  verify_device   cda_nmt_verify_device of those proofs (everything in device memory)
  verify_host     cda_nmt_verify of the same proofs through host buffers
One JSON line.  python scripts/sampling_probe.py [reps]   (DESIGN.md §16 holds the recorded figures)"""
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
k, w, mn = 128, 256, 16
nq = w * w
ctx = cda.Context(0)
ods = bench.gen_ods(k, 0xC0FFEE)
dev = torch.device("cuda", 0)


def median_ms(f, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


out = {"k": k, "proofs": nq, "reps": reps}
out["open_ms"] = median_ms(lambda: ctx.open_square(ods).close())

q = np.zeros(nq, N.RANGE_QUERY_DTYPE)
q["index"], q["start"] = np.divmod(np.arange(nq, dtype=np.uint32), w)
q["end"] = q["start"] + 1
sq = ctx.open_square(ods)
counts = np.zeros(nq, np.int32)
nodes = np.zeros((nq, mn, N.NODE_SIZE), np.uint8)
shares = np.zeros((nq, N.SHARE_SIZE), np.uint8)
L = ctx._L


def prove(with_cells):
    rc = L.cda_square_prove(sq._h, nq, N._p(q), mn, N._p(counts), N._p(nodes), N._p(shares) if with_cells else None,
                            shares.nbytes if with_cells else 0)
    assert rc == 0, rc


out["prove_cells_ms"] = median_ms(lambda: prove(True))
out["prove_nodes_only_ms"] = median_ms(lambda: prove(False))
out["prove_cells_bytes"] = int(counts.nbytes + nodes.nbytes + shares.nbytes)
out["prove_nodes_only_bytes"] = int(counts.nbytes + nodes.nbytes)
prove(True)
assert (counts == 8).all()

descs = np.zeros(nq, N.NMT_PROOF_DESC_DTYPE)
descs["start"], descs["end"] = q["start"], q["end"]
descs["node_off"] = np.arange(nq, dtype=np.uint32) * mn
descs["nnodes"] = counts
descs["leaf_off"] = np.arange(nq, dtype=np.uint32)
descs["root"] = q["index"]
ns = np.full((nq, N.NAMESPACE_SIZE), 0xFF, np.uint8)
q0 = (q["index"] < k) & (q["start"] < k)
ns[q0] = ods.reshape(k, k, N.SHARE_SIZE)[:, :, :N.NAMESPACE_SIZE].reshape(-1, N.NAMESPACE_SIZE)
roots = np.concatenate([sq.row_roots, sq.col_roots])
flat_nodes = nodes.reshape(-1, N.NODE_SIZE)

ok = ctx.nmt_verify(descs, ns, roots, flat_nodes, shares)
assert ok.all(), int(ok.sum())
out["verify_host_ms"] = median_ms(lambda: ctx.nmt_verify(descs, ns, roots, flat_nodes, shares))
out["verify_host_bytes"] = int(descs.nbytes + ns.nbytes + roots.nbytes + flat_nodes.nbytes + shares.nbytes)

d = {n: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
     for n, a in (("descs", descs), ("ns", ns), ("roots", roots), ("nodes", flat_nodes), ("leaves", shares))}
d_ok = torch.zeros(nq, dtype=torch.uint8, device=dev)
stream = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def verify_device():
    ctx.nmt_verify_device(nq, d["descs"].data_ptr(), d["ns"].data_ptr(), d["roots"].data_ptr(), len(roots),
                          d["nodes"].data_ptr(), len(flat_nodes), d["leaves"].data_ptr(), nq, d_ok.data_ptr(),
                          stream.cuda_stream)
    stream.synchronize()


out["verify_device_ms"] = median_ms(verify_device)
assert bool(d_ok.all())
# the launches alone (HIP events around both kernels: the one-leaf proofs' and the range kernel's empty pass)
ctx.profile_enable(True)
ctx.profile_reset()
for _ in range(reps):
    verify_device()
ms, n = ctx.profile_read().get("nmt_verify", (0.0, 0))
ctx.profile_enable(False)
out["verify_device_kernels_ms"] = round(ms / max(n, 1), 3)
# the same proofs four times over (descriptors and namespaces repeated; nodes, cells and roots shared): 65,536 proofs
# are 1,024 waves, one per SIMD of the device, and four per SIMD is what the SHA-256 ceiling is measured at
d4 = {n: d[n].repeat(4) for n in ("descs", "ns")}
d_ok4 = torch.zeros(4 * nq, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def verify_device_x4():
    ctx.nmt_verify_device(4 * nq, d4["descs"].data_ptr(), d4["ns"].data_ptr(), d["roots"].data_ptr(), len(roots),
                          d["nodes"].data_ptr(), len(flat_nodes), d["leaves"].data_ptr(), nq, d_ok4.data_ptr(),
                          stream.cuda_stream)
    stream.synchronize()


out["verify_device_x4_ms"] = median_ms(verify_device_x4)
assert bool(d_ok4.all())
out["verify_device_x4_gcomp_s"] = round(4 * nq * 33 / out["verify_device_x4_ms"] / 1e6, 2)
out["verify_device_x4_fraction_of_28.7"] = round(out["verify_device_x4_gcomp_s"] / 28.7, 3)
# a one-cell proof of a 256-leaf tree: 9 leaf compressions + 8 nodes of 3
compressions = nq * (9 + 8 * 3)
out["compressions"] = compressions
out["verify_device_gcomp_s"] = round(compressions / out["verify_device_ms"] / 1e6, 2)
out["verify_device_fraction_of_28.7"] = round(out["verify_device_gcomp_s"] / 28.7, 3)
out["prove_cells_gb_s"] = round(out["prove_cells_bytes"] / out["prove_cells_ms"] / 1e6, 1)
out["verify_host_gb_s"] = round(out["verify_host_bytes"] / out["verify_host_ms"] / 1e6, 1)
sq.close()
ctx.close()
print(json.dumps(out))
