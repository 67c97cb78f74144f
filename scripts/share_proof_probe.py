"""Share proofs to the data root at the workload's own size (k = 128): medians over `reps` repetitions after warm-up of
  open                 cda_square_open (extend + commit, every tree node and the data-root tree retained)
  prove_256x64         ONE cda_square_share_proofs call for 256 ranges of 64 shares, into host buffers
  prove_rows           ONE call for the 128 whole rows
  prove_cells          ONE call for all 16,384 shares as ranges of their own (the gather kernel with the device full)
  loop_*               the same ranges through a loop of cda_share_inclusion_proof (one extension per proof)
  validate_device_*    cda_share_proofs_validate_device on those proofs, everything in device memory
  nmt_verify_device_*  cda_nmt_verify_device on the same row records: the NMT leg alone
and the launches alone (HIP events around the kernels, cda_profile_*).  One JSON line.
  python scripts/share_proof_probe.py [reps]          (DESIGN.md §17 holds the recorded figures)
  python scripts/share_proof_probe.py [reps] open     only the open (runs against any build: CDA_LIB)"""
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
k = 128
ctx = cda.Context(0)
ods = bench.gen_ods(k, 0xC0FFEE).copy()
ods[:, :N.NAMESPACE_SIZE] = ods[0, :N.NAMESPACE_SIZE]  # one namespace: every range is a proof that validates
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


def kernels_ms(f, *names):
    """Mean per call of the named profile scopes (HIP events around the launches) over `reps` calls of f."""
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

rng = np.random.default_rng(17)
workloads = {
    "256x64": [(int(s), int(s) + 64) for s in rng.integers(0, k * k - 64, 256)],
    "rows": [(r * k, (r + 1) * k) for r in range(k)],
}
sq = ctx.open_square(ods)
mn, na = sq.max_nodes, (4 * k).bit_length() - 1
stream = torch.cuda.Stream(dev)
for name, ranges in workloads.items():
    nrows, nshares = sq.share_proof_sizes(k, ranges)
    out[f"{name}_row_records"], out[f"{name}_shares"] = nrows, nshares
    out[f"prove_{name}_ms"] = median_ms(lambda: sq.share_proofs_raw(ranges))
    out[f"prove_{name}_kernel_ms"], = kernels_ms(lambda: sq.share_proofs_raw(ranges), "square_share_proofs")
    # what the gather kernel moves: every output byte is read once from the retained square and written once
    moved = 2 * (nrows * (N.SHARE_ROW_DTYPE.itemsize // 2 + mn * N.NODE_SIZE + N.NODE_SIZE + 32 + na * 32) +
                 nshares * N.SHARE_SIZE)
    out[f"prove_{name}_kernel_gb_s"] = round(moved / out[f"prove_{name}_kernel_ms"] / 1e6, 1)
    out[f"loop_{name}_ms"] = median_ms(lambda: [ctx.share_inclusion_proof(ods, s, e) for s, e in ranges], warm=1)
    out[f"loop_over_batched_{name}"] = round(out[f"loop_{name}_ms"] / out[f"prove_{name}_ms"], 1)

    # validate on the device: the proofs as cda_square_share_proofs wrote them, descriptors from the ranges
    raw = sq.share_proofs_raw(ranges)
    descs = np.zeros(len(ranges), N.SHARE_PROOF_DESC_DTYPE)
    leaf = 0
    for i, (s, e) in enumerate(ranges):
        lo, n = int(raw["row_off"][i]), int(raw["row_off"][i + 1] - raw["row_off"][i])
        descs[i] = (lo, n, n, n, leaf, e - s, s // k, (e - 1) // k, 0, ods[0, :N.NAMESPACE_SIZE], 0)
        leaf += e - s
    nmt = np.zeros(nrows, N.NMT_PROOF_DESC_DTYPE)
    nmt["start"], nmt["end"] = raw["rows"]["nmt_start"], raw["rows"]["nmt_end"]
    nmt["node_off"], nmt["nnodes"] = raw["rows"]["node_off"], raw["rows"]["nnodes"]
    nmt["leaf_off"] = np.concatenate([[0], np.cumsum(nmt["end"] - nmt["start"])[:-1]])
    nmt["root"] = np.arange(nrows)
    ns = np.repeat(ods[:1, :N.NAMESPACE_SIZE], nrows, 0)
    d = {n: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
         for n, a in (("descs", descs), ("rows", raw["rows"]), ("row_roots", raw["row_roots"]),
                      ("leaf_hashes", raw["leaf_hashes"]), ("nodes", raw["nodes"]), ("aunts", raw["aunts"]),
                      ("shares", raw["shares"]), ("root", np.frombuffer(raw["data_root"], np.uint8)),
                      ("nmt", nmt), ("ns", ns))}
    d_verdicts = torch.full((len(ranges),), -1, dtype=torch.int32, device=dev)
    d_ok = torch.zeros(nrows, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def validate_device():
        ctx.share_proofs_validate_device(len(ranges), d["descs"].data_ptr(), d["rows"].data_ptr(),
                                         d["row_roots"].data_ptr(), d["leaf_hashes"].data_ptr(), nrows,
                                         d["nodes"].data_ptr(), nrows * mn, d["aunts"].data_ptr(), nrows * na,
                                         d["shares"].data_ptr(), nshares, d["root"].data_ptr(), 1,
                                         d_verdicts.data_ptr(), stream.cuda_stream)
        stream.synchronize()

    def nmt_verify_device():
        ctx.nmt_verify_device(nrows, d["nmt"].data_ptr(), d["ns"].data_ptr(), d["row_roots"].data_ptr(), nrows,
                              d["nodes"].data_ptr(), nrows * mn, d["shares"].data_ptr(), nshares, d_ok.data_ptr(),
                              stream.cuda_stream)
        stream.synchronize()

    out[f"validate_device_{name}_ms"] = median_ms(validate_device)
    assert not bool(d_verdicts.any()), d_verdicts.cpu().numpy()
    out[f"nmt_verify_device_{name}_ms"] = median_ms(nmt_verify_device)
    assert bool(d_ok.all())
    out[f"validate_device_{name}_kernels_ms"], = kernels_ms(validate_device, "share_proofs_validate")
    out[f"nmt_verify_device_{name}_kernels_ms"], = kernels_ms(nmt_verify_device, "nmt_verify")
    # the row-proof leg: 2 compressions for the leaf hash and 2 per aunt, a lane per row record
    out[f"row_proof_compressions_{name}"] = nrows * (2 + 2 * na)
    out[f"validate_host_{name}_ms"] = median_ms(lambda: ctx.share_proofs_validate(
        descs, raw["rows"], raw["row_roots"], raw["leaf_hashes"], raw["nodes"], raw["aunts"], raw["shares"],
        np.frombuffer(raw["data_root"], np.uint8)))
# the gather kernel at a size that fills the device: every share of the square as a range of its own
cells = [(i, i + 1) for i in range(k * k)]
out["prove_cells_ms"] = median_ms(lambda: sq.share_proofs_raw(cells))
out["prove_cells_kernel_ms"], = kernels_ms(lambda: sq.share_proofs_raw(cells), "square_share_proofs")
moved = 2 * k * k * (N.SHARE_ROW_DTYPE.itemsize // 2 + mn * N.NODE_SIZE + N.NODE_SIZE + 32 + na * 32 + N.SHARE_SIZE)
out["prove_cells_kernel_gb_s"] = round(moved / out["prove_cells_kernel_ms"] / 1e6, 1)
sq.close()
ctx.close()
print(json.dumps(out))
