"""What tests/test_blob_index.py (CPU), tests/test_blob_index_gpu.py and scripts/blob_probe.py share: tx sets that
square.construct lays out at a wanted square size, the k = 128 mix of 32 blobs placed by NextShareIndex, the alphabet
of the rule dump and the named mutations that give each status bit of cda_square_index.
"""
import functools

import numpy as np

from cda import _native as N
from cda import blob as B
from cda import inclusion as I
from cda import square as S

SHARE = 512


def blob_ns(i):
    """A version-0 namespace above the reserved ones, ascending with i."""
    return bytes(19) + b"\x01" + int(i).to_bytes(9, "big")


def blob_tx(tx, blobs):
    """blob.MarshalBlobTx: BlobTx{tx=1, blobs=2, type_id=3 "BLOB"}; blobs: (29-byte namespace, data)."""
    out = b"\x0a" + S.varint(len(tx)) + tx
    for ns, data in blobs:
        b = b"\x0a" + S.varint(28) + ns[1:] + b"\x12" + S.varint(len(data)) + data
        out += b"\x12" + S.varint(len(b)) + b
    return out + b"\x1a\x04BLOB"


# square size -> (sizes of the normal txs, per BlobTx the sizes of its blobs)
SYNTHETIC = {
    1: ([100], []),                                    # no blobs
    2: ([], [[300]]),                                  # no normal txs
    4: ([200, 700], [[1500, 100], [900]]),
    8: ([300, 300], [[1500, 100], [3000], [9000, 1]]),
    16: ([5000, 40, 900], [[20000, 478], [479, 959, 960, 961], [30000], [1]]),
}


@functools.lru_cache(maxsize=None)
def synthetic_txs(k):
    rng = np.random.default_rng(0xB10B + k)
    normal, blob_txs = SYNTHETIC[k]
    txs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in normal]
    nsid = 1
    for sizes in blob_txs:
        blobs = []
        for n in sizes:
            # namespaces neither ascending nor distinct per tx: construct sorts them
            blobs.append((blob_ns(1 + (nsid * 7) % 5), rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            nsid += 1
        txs.append(blob_tx(rng.integers(0, 256, 120, dtype=np.uint8).tobytes(), blobs))
    return tuple(txs)


def ods_array(shares):
    return np.frombuffer(b"".join(bytes(s) for s in shares), np.uint8).reshape(-1, SHARE).copy()


@functools.lru_cache(maxsize=None)
def synthetic_square(k):
    """-> (ods, layout info) of square.construct(synthetic_txs(k)); the square size is k."""
    ss, shares, info = S.construct(list(synthetic_txs(k)), 128, 64)
    assert ss == k, (ss, k)
    return ods_array(shares), info


@functools.lru_cache(maxsize=None)
def long_blob_square():
    """k = 64 with one blob from share 64 to past share 2,304."""
    rng = np.random.default_rng(0xB164)
    data = rng.integers(0, 256, 478 + 482 * 2299, dtype=np.uint8).tobytes()
    txs = [rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), blob_tx(b"pfb" * 30, [(blob_ns(9), data)])]
    ss, shares, info = S.construct(txs, 128, 64)
    assert ss == 64 and info["first_blob"] < 256 and info["first_blob"] + 2300 > 2304
    return ods_array(shares)


@functools.lru_cache(maxsize=None)
def mix_square(k=128, threshold=64, seed=408):
    """The k = 128 mix of DESIGN §23 with real shares: a TRANSACTION and a PAY_FOR_BLOB sequence in the first 16
    shares, then blobs of 1 .. 3,000 shares, each under a namespace of its own, placed by NextShareIndex until the
    square is full -> (ods, [(start, nshares, namespace, data)])."""
    sizes, rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    # scripts/commitment_probe.py draws its shares from this generator before the sizes: the same 32 sizes here
    sizes.integers(0, 256, (k * k, SHARE), dtype=np.uint8)
    shares = S.compact_shares(S.TX_NAMESPACE, [rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()])
    shares += S.compact_shares(S.PAY_FOR_BLOB_NAMESPACE, [rng.integers(0, 256, 700, dtype=np.uint8).tobytes()])
    assert len(shares) <= 16
    shares += [S.padding_share(S.PRIMARY_RESERVED_PADDING_NAMESPACE)] * (16 - len(shares))
    blobs, prev_ns = [], S.PRIMARY_RESERVED_PADDING_NAMESPACE
    while True:
        n = int(sizes.choice([1, 2, 5, 17, 64, 129, 352, 1000, 3000]))
        start = I.next_share_index(len(shares), n, threshold)
        if start + n > k * k:
            break
        size = 1 if n == 1 and rng.random() < 0.5 else 478 + 482 * (n - 1) - int(rng.integers(0, 482 if n > 1 else 478))
        assert I.sparse_shares_needed(size) == n
        ns, data = blob_ns(len(blobs) + 1), rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        shares += [S.padding_share(prev_ns)] * (start - len(shares))
        shares += S.sparse_shares(ns, data)
        blobs.append((start, n, ns, data))
        prev_ns = ns
    shares += [S.padding_share(S.TAIL_PADDING_NAMESPACE)] * (k * k - len(shares))
    return ods_array(shares), blobs


def oracle_commit(threshold=64):
    """CreateCommitment by the CPU oracle, in index_host's `commit` form."""
    import oracle_lib as O

    def commit(ns, data, version):
        rc, out = O.blob_commitment(ns, data, version, threshold)
        assert rc == 0
        return out
    return commit


# ---- the rule dump's alphabet: bytes [0, 34) of a share ----
def head(ns, version=0, start=True, seq_len=0):
    return bytes(ns) + bytes([version << 1 | (1 if start else 0)]) + int(seq_len).to_bytes(4, "big")


ALPHABET = [
    ("blob start, 1 byte", head(blob_ns(1), seq_len=1)),
    ("blob start, 479 bytes", head(blob_ns(1), seq_len=479)),
    ("blob start, 2000 bytes", head(blob_ns(1), seq_len=2000)),
    ("continuation, same namespace", head(blob_ns(1), start=False, seq_len=0x01020304)),
    ("continuation, another namespace", head(blob_ns(2), start=False)),
    ("padding", head(blob_ns(1))),
    ("version-1 start", head(blob_ns(1), version=1, seq_len=479)),
    ("TX start", head(S.TX_NAMESPACE, seq_len=475)),
    ("reserved-namespace start", head(bytes(28) + b"\x09", seq_len=1)),
    ("empty PFB start", head(S.PAY_FOR_BLOB_NAMESPACE)),
    # lengths whose share count wraps in 32-bit arithmetic (from 0xFFFFFFFD on): 8,910,721 and 8,985,288 shares
    ("blob start, 0xFFFFFFFF bytes", head(blob_ns(1), seq_len=0xFFFFFFFF)),
    ("TX start, 0xFFFFFFFF bytes", head(S.TX_NAMESPACE, seq_len=0xFFFFFFFF)),
]


# ---- hostile squares: named mutations of a valid square ----
def _blobs(ods, k):
    seqs, _, _ = B.index_host(list(ods), k, 64, commit=False)
    return seqs[seqs["kind"] == N.SEQ_KIND_BLOB]


def _set_len(ods, share, seq_len):
    ods[share, 30:34] = np.frombuffer(int(seq_len).to_bytes(4, "big"), np.uint8)


def _mut_truncated(case):
    ods, k = case["ods"], case["k"]
    _set_len(ods, int(_blobs(ods, k)[-1]["start"]), 482 * k * k)


def _mut_broken(case):
    ods = case["ods"]
    b = next(b for b in _blobs(ods, case["k"]) if b["nshares"] >= 4)
    ods[int(b["start"]) + 2, 29] |= 1  # a continuation share in its middle becomes a start share


def _mut_version(case):
    ods = case["ods"]
    b = next(b for b in _blobs(ods, case["k"]) if b["nshares"] >= 4)
    ods[int(b["start"]):int(b["start"]) + int(b["nshares"]), 29] |= 2  # share version 1 throughout


def _mut_reserved(case):
    ods = case["ods"]
    b = _blobs(ods, case["k"])[0]  # the first blob takes the namespace of the padding before it: the order stays
    ns = np.frombuffer(S.PRIMARY_RESERVED_PADDING_NAMESPACE, np.uint8)
    ods[int(b["start"]):int(b["start"]) + int(b["nshares"]), :29] = ns


def _mut_threshold(case):
    case["threshold"] = 1  # W grows to 2 and more while the blobs stay where threshold 64 put them


# (name, the status bit it must produce, the mutation)
MUTATIONS = [
    ("last blob's length past the square", N.SEQ_TRUNCATED, _mut_truncated),
    ("start bit in a blob's middle", N.SEQ_BROKEN, _mut_broken),
    ("share version one", N.SEQ_VERSION, _mut_version),
    ("first blob in the reserved padding namespace", N.SEQ_RESERVED_NS, _mut_reserved),
    ("threshold one", N.SEQ_UNALIGNED, _mut_threshold),
]


def mutated(k, *names):
    """{"ods", "k", "threshold"} of synthetic_square(k) with the named mutations applied in order."""
    case = {"ods": synthetic_square(k)[0].copy(), "k": k, "threshold": 64}
    for name in names:
        next(fn for n, _, fn in MUTATIONS if n == name)(case)
    return case


def orphan_run_square(k=8):
    """The TRANSACTION sequence's start share turned into a continuation share: an orphan run from share 0."""
    ods = synthetic_square(k)[0].copy()
    ods[0, 29] &= 0xFE
    return ods


def continuation_only_square(k=8):
    ods = synthetic_square(k)[0].copy()
    ods[:, 29] &= 0xFE
    return ods


def huge_length_squares(k=8):
    """Blob and compact start shares whose seq_len is 0xFFFFFFFE / 0xFFFFFFFF: the claim is millions of shares."""
    blob = synthetic_square(k)[0].copy()
    _set_len(blob, int(_blobs(blob, k)[1]["start"]), 0xFFFFFFFE)
    both = blob.copy()
    _set_len(both, 0, 0xFFFFFFFF)  # the TRANSACTION sequence's start share
    _set_len(both, int(_blobs(both, k)[0]["start"]), 0xFFFFFFFF)
    return blob, both
