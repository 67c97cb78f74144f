"""Reading a retained square back at k = 128 on DESIGN §23's mix with real shares (tests/blob_cases.py mix_square: a
TRANSACTION and a PAY_FOR_BLOB sequence, 32 blobs of 1 to 3,000 shares placed by NextShareIndex): medians over `reps`
repetitions after 3 warm-up calls, the routes of a comparison run in turn in one process.
  (a) index_ms              Square.index with the commitments; index_only_ms without them; commitments_ms the
                            commitments-only call on the ranges the index found (what the second wait carries)
  (b) read_host_ms / read_device_ms   every blob's payload in one cda_square_read call, to host and to device memory,
                            with the kernel's time by HIP events and its rate (share bytes read + payload bytes
                            written) against the copy kernel's (tools/libcopybw.so); on the library given as
                            the third argument (a -DCDA_BLOB_GATHER_BYTEWISE=1 build: make BUILD=build_bw OUT=... EXTRA=...)
                            the same for the bytewise gather
  (c) get_ms                blob.get of one blob by namespace and commitment, end to end
      before_*_ms           the route before: namespace.get_shares_by_namespace per namespace and a host strip of the
                            returned shares, on the library given as the second argument (the parent commit's build),
                            else on this one
One JSON line, also written to the file given as the fourth argument.
  python scripts/blob_probe.py [reps] [parent libcda.so] [bytewise-gather libcda.so] [out.json]   """
import json
import os
import sys
import time

import numpy as np
import torch  # first: libcda then resolves HIP through torch's runtime, as in bench.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blob_cases as K  # noqa: E402
import cda  # noqa: E402
from cda import _native as N  # noqa: E402
from cda import blob as B  # noqa: E402
from cda import namespace as NS  # noqa: E402

arg = lambda i: sys.argv[i] if len(sys.argv) > i and sys.argv[i] not in ("", "-") else None  # noqa: E731
reps = int(arg(1) or 15)
parent, other, out_path = arg(2), arg(3), arg(4)
k, threshold = 128, 64
dev = torch.device("cuda", 0)
ctx = cda.Context(0)
for path in (parent, other):
    if path:
        N.lib(path, older=True)
old = cda.Context(0, lib_path=parent) if parent else ctx
ods, blobs = K.mix_square()
sq = ctx.open_square(ods)
old_sq = old.open_square(ods) if parent else sq
state = {}


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def median_alternating(fs, warm=3):
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


seqs, com, summary = sq.index(threshold)
found = seqs[seqs["kind"] == N.SEQ_KIND_BLOB]
ranges = [(int(s["start"]), int(s["nshares"])) for s in found]
q = sq.sequence_ranges(found)
payload = int(found["seq_len"].sum())
offs = np.zeros(len(q), np.uint64)
offs[1:] = np.cumsum(found["seq_len"].astype(np.uint64))[:-1]
d_out = torch.zeros(payload, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
moved = int(found["nshares"].sum()) * 512 + payload  # share bytes the gather touches + payload bytes written


def index():
    state["index"] = sq.index(threshold)


def index_only():
    sq.index(threshold, commitments=False)


def commitments():
    state["com"] = sq.commitments(ranges, threshold)


def read_host():
    state["host"] = sq.read(q)


def read_device(s=sq, d=d_out):
    s.read_device(q, offs, payload, d.data_ptr())


def get():
    state["get"] = B.get(sq, blobs[20][2], com[2 + 20].tobytes(), threshold)


def strip_rows(rows):
    shares = [s for _, row, _ in rows for s in row]
    n = int.from_bytes(shares[0][30:34], "big")
    return b"".join([shares[0][34:]] + [s[30:] for s in shares[1:]])[:n]


def before_all():
    state["before"] = [strip_rows(NS.get_shares_by_namespace(old_sq, b[2])) for b in blobs]


def before_one():
    state["before_one"] = strip_rows(NS.get_shares_by_namespace(old_sq, blobs[20][2]))


out = {"k": k, "threshold": threshold, "reps": reps, "blobs": len(blobs), "blob_shares": int(found["nshares"].sum()),
       "payload_bytes": payload, "moved_bytes": moved, "nseq": summary["nseq"], "build": N.build_info(),
       "parent_build": N.build_info(parent) if parent else "this library"}
out["index_ms"], out["index_only_ms"], out["commitments_ms"] = median_alternating([index, index_only, commitments])
assert [x.tobytes() for x in state["index"][1][2:]] == state["com"]
out["read_host_ms"], out["read_device_ms"], out["before_all_ms"] = median_alternating([read_host, read_device, before_all])
assert state["host"] == [b[3] for b in blobs] == state["before"]
assert d_out.cpu().numpy().tobytes() == b"".join(b[3] for b in blobs)
out["get_ms"], out["before_one_ms"] = median_alternating([get, before_one])
assert state["get"].data == blobs[20][3] == state["before_one"]
out["index_kernels_ms"] = kernels_ms(ctx, index)
out["read_kernels_ms"] = kernels_ms(ctx, read_device)
gather_ms = out["read_kernels_ms"]["square_read"]
out["gather_gbs"] = round(moved / gather_ms / 1e6, 1)
out["read_device_gbs"] = round(moved / out["read_device_ms"] / 1e6, 1)
out["read_host_gbs"] = round(payload / out["read_host_ms"] / 1e6, 2)  # payload bytes delivered to host memory
if other:
    alt = cda.Context(0, lib_path=other)
    alt_sq = alt.open_square(ods)
    d_alt = torch.zeros(payload, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    f = lambda: read_device(alt_sq, d_alt)  # noqa: E731
    out["read_device_ms_ab"], out["read_device_bytewise_ms"] = median_alternating([read_device, f])
    assert d_alt.cpu().numpy().tobytes() == b"".join(b[3] for b in blobs)
    out["bytewise_build"] = N.build_info(other)
    out["bytewise_gather_ms"] = kernels_ms(alt, f)["square_read"]
    alt_sq.close()
    alt.close()
# the copy kernel's rate on this box, live in this process (tools/copy_bw.hip, as bench.py measures it)
import ctypes  # noqa: E402
tool = os.path.join(ROOT, "tools", "libcopybw.so")
if os.path.exists(tool):
    L = ctypes.CDLL(tool)
    L.copybw_measure.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    rates, cfg = (ctypes.c_double * 3)(), (ctypes.c_int * 3)()
    if L.copybw_measure(0, 1 << 30, 10, rates, cfg) == 0:
        out["copy_ceiling_gbs"] = round(rates[0], 1)
        out["gather_fraction_of_copy"] = round(out["gather_gbs"] / rates[0], 3)
sq.close()
if old is not ctx:
    old_sq.close()
    old.close()
ctx.close()
line = json.dumps(out)
print(line)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
