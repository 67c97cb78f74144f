"""CPU tests of the bad-encoding fraud proof rule: cda.befp.validate_host on honest and one-cell-
corrupted squares under both decoders of the oracle, one mutation per verdict code, plan::befp_precheck (what the prep
kernel of cda_befp_validate evaluates) under ASan and UBSan against a Python restatement, and the C ABI's argument
checks.  The squares' trees, roots and proofs here are the host wrapper tree's (hashlib); tests/test_befp_gpu.py holds
the device side."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from cda import _native as N
from cda import befp
from cda.befp import BAD_SHARE, FRAUD, MALFORMED, NO_FRAUD, TOO_FEW, BadEncodingProof
from cda.wrapper import ErasuredNamespacedMerkleTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")
NS = N.NAMESPACE_SIZE


class OracleCodec:
    """The oracle's codec as validate_host takes one: fft = False the Lagrange decoder, True its Leopard decoder."""

    def __init__(self, fft):
        self.fft = fft

    def encode(self, data):
        return [bytes(x) for x in O.leo_encode(np.stack([np.frombuffer(bytes(x), np.uint8) for x in data]))]

    def decode(self, shards):
        arr = np.zeros((len(shards), N.SHARE_SIZE), np.uint8)
        present = np.zeros(len(shards), np.uint8)
        for i, x in enumerate(shards):
            if x is not None:
                arr[i] = np.frombuffer(x, np.uint8)
                present[i] = 1
        rc, out = O.leo_decode(arr, present, fft=self.fft)
        assert rc == 0
        return [bytes(r) for r in out]


CODECS = {"lagrange": OracleCodec(False), "leopard": OracleCodec(True)}


class HostSquare:
    """A 2k x 2k square as committed, on the host: its 4k wrapper trees, their roots and cell proofs (hashlib)."""

    def __init__(self, eds, k):
        self.k, self.w = k, 2 * k
        self.grid = np.ascontiguousarray(eds, np.uint8).reshape(self.w, self.w, N.SHARE_SIZE)
        self.trees, self._proofs = {}, {}
        for axis in (0, 1):
            for i in range(self.w):
                t = ErasuredNamespacedMerkleTree(k, i)
                t._leaves = [bytes(x) for x in (self.grid[:, i] if axis else self.grid[i])]
                self.trees[axis, i] = t
        self.row_roots = [self.trees[0, i]._root_node() for i in range(self.w)]
        self.col_roots = [self.trees[1, i]._root_node() for i in range(self.w)]

    @property
    def roots(self):
        return self.row_roots, self.col_roots

    def cell(self, axis, index, pos):
        return bytes(self.grid[pos, index] if axis else self.grid[index, pos])

    def prove(self, axis, index, leaf):
        key = (axis, index, leaf)
        if key not in self._proofs:
            self._proofs[key] = self.trees[axis, index].prove_range(leaf, leaf + 1)
        return self._proofs[key]

    def create(self, axis, index, positions=None):
        """befp.create's result from the host trees: every cell proved in its orthogonal tree."""
        positions = range(self.w) if positions is None else sorted(positions)
        return BadEncodingProof(axis, index, [(p, self.cell(axis, index, p), self.prove(1 - axis, p, index))
                                              for p in positions])


def honest_eds(k, seed):
    return O.extend(O.gen_ods(k, seed))


def position_sets(k, rng, contain=None, avoid=None):
    """Position sets of k, k + 1 and 2k shares of an axis of 2k cells (those that exist), with `contain` in or `avoid`
    out of the first two."""
    w, out = 2 * k, []
    for n in sorted({k, min(k + 1, 2 * k)}):
        pool = [p for p in range(w) if p not in (contain, avoid)]
        need = n - (contain is not None)
        if need > len(pool) or (n == w and avoid is not None):
            continue
        pick = sorted(int(x) for x in rng.choice(pool, need, replace=False)) if need else []
        out.append(sorted(pick + ([contain] if contain is not None else [])))
    if avoid is None:
        out.append(list(range(w)))
    return out


def both(proof, sq, want=None):
    """validate_host under both decoders: equal verdicts (and `want`)."""
    got = {name: befp.validate_host(proof, *sq.roots, codec=c) for name, c in CODECS.items()}
    assert got["lagrange"] == got["leopard"], got
    if want is not None:
        assert got["lagrange"] == want, (got, proof.axis, proof.index, [p for p, _, _ in proof.shares])
    return got["lagrange"]


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_honest_square_is_never_fraud(k):
    sq = HostSquare(honest_eds(k, 0xBE00 + k), k)
    rng = np.random.default_rng(k)
    for axis in (0, 1):
        for index in range(2 * k):
            for pos in position_sets(k, rng):
                both(sq.create(axis, index, pos), sq, NO_FRAUD)


def corruptions(k):
    """(name, row, col, byte): one cell of each parity quadrant, a Q0 payload byte, and a namespace byte of the last
    Q0 cell."""
    w = 2 * k
    return [("q1", 0, k, 100), ("q2", w - 1, 0, 200), ("q3", k, w - 1, 511), ("q0-payload", 0, k - 1, 300),
            ("q0-namespace", k - 1, k - 1, NS - 1)]


def corrupted(eds, k, row, col, byte):
    bad = np.array(eds, copy=True).reshape(2 * k, 2 * k, N.SHARE_SIZE)
    bad[row, col, byte] ^= 0x01
    return bad.reshape(-1, N.SHARE_SIZE)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_one_cell_corruption(k):
    """The two axes through a corrupted cell are FRAUD whichever shares are chosen (the committed root is over a
    non-codeword): sets that hold the cell, sets that leave it out, and all 2k, where only the re-encode exposes a bad
    parity cell.  The neighbouring axes are NO_FRAUD.  Both decoders agree on every verdict."""
    eds = honest_eds(k, 0xBE10 + k)
    w = 2 * k
    for name, row, col, byte in corruptions(k):
        sq = HostSquare(corrupted(eds, k, row, col, byte), k)
        rng = np.random.default_rng(row * w + col)
        for axis, index, pos in ((0, row, col), (1, col, row)):
            sets = position_sets(k, rng, contain=pos) + position_sets(k, rng, avoid=pos)
            assert any(pos in s for s in sets) and any(pos not in s for s in sets) and list(range(w)) in sets
            for s in sets:
                both(sq.create(axis, index, s), sq, FRAUD)
            for s in position_sets(k, rng):
                both(sq.create(axis, (index + 1) % w, s), sq, NO_FRAUD)
                both(sq.create(axis, (index - 1) % w, s), sq, NO_FRAUD)


def test_fraud_reason_depends_on_the_decoder_the_verdict_does_not():
    """k = 2, cell (1, 1) byte 3 (a namespace byte), three shares: the rebuilt Q0 namespaces are garbage, and whether
    the tree stops at the push order or ends in another root is the decoder's; FRAUD either way."""
    k = 2
    sq = HostSquare(corrupted(honest_eds(k, 0xBE22), k, 1, 1, 3), k)
    reasons = set()
    for axis in (0, 1):
        for s in ([0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]):
            why = {}
            for name, c in CODECS.items():
                r = []
                assert befp.validate_host(sq.create(axis, 1, s), *sq.roots, codec=c, reason=r) == FRAUD
                why[name] = r[0]
            reasons |= set(why.values())
    assert reasons == {"order", "root"}


def test_one_mutation_per_verdict_code():
    k, w = 4, 8
    sq = HostSquare(honest_eds(k, 0xBE30), k)
    base = sq.create(0, 2)
    both(base, sq, NO_FRAUD)

    def mutated(**kw):
        p = BadEncodingProof(base.axis, base.index, list(base.shares))
        for name, v in kw.items():
            setattr(p, name, v)
        return p
    sh = base.shares
    both(mutated(axis=2), sq, MALFORMED)
    both(mutated(index=w), sq, MALFORMED)
    both(mutated(shares=sh[:-1] + [(w,) + sh[-1][1:]]), sq, MALFORMED)
    both(mutated(shares=sh[:3] + [sh[2]] + sh[4:]), sq, MALFORMED)             # a duplicated position
    both(mutated(shares=sh[:3] + [sh[4], sh[3]] + sh[5:]), sq, MALFORMED)       # two positions swapped
    both(mutated(shares=sh + [sh[-1]]), sq, MALFORMED)                          # 2k + 1 shares
    both(mutated(shares=sh[:k - 1]), sq, TOO_FEW)
    both(mutated(shares=[(w, sh[0][1], sh[0][2])] + sh[1:k - 1]), sq, MALFORMED)  # B1 before B2
    pos, share, nmt = sh[5]
    flipped = bytes([share[0]]) + bytes([share[1] ^ 0x80]) + share[2:]
    both(mutated(shares=sh[:5] + [(pos, flipped, nmt)] + sh[6:]), sq, BAD_SHARE)
    dropped = type(nmt)(nmt.start, nmt.end, nmt.nodes[:-1])
    both(mutated(shares=sh[:5] + [(pos, share, dropped)] + sh[6:]), sq, BAD_SHARE)
    wrong_leaf = sq.prove(1, pos, 3)  # the column's proof of row 3's cell, not row 2's
    both(mutated(shares=sh[:5] + [(pos, share, wrong_leaf)] + sh[6:]), sq, BAD_SHARE)
    own_axis = sq.prove(0, 2, pos)    # against the row's own root instead of the column's
    both(mutated(shares=sh[:5] + [(pos, share, own_axis)] + sh[6:]), sq, BAD_SHARE)
    # a Q0 share under another namespace still hashes as a leaf of its own namespace: rejected by the column's root
    pos, share, nmt = sh[1]
    other_ns = bytes([share[0]]) + bytes([share[1] ^ 1]) + share[2:]
    both(mutated(shares=[sh[0], (pos, other_ns, nmt)] + sh[2:]), sq, BAD_SHARE)


# ---- plan::befp_precheck against a restatement ----
def precheck_mirror(k, descs, entries, shares, nnodes_total, nroots):
    """B1, B2 and the prep step's outputs, restated: the lines tests/san/befp_rule_dump.cpp prints."""
    w, lines = 2 * k, []
    empty = ("0 0 0 0 0 0 " + "00" * NS, )
    for axis, index, entry_off, nshares, root_off in descs:
        ok = axis <= 1 and index < w and nshares <= w and entry_off + nshares <= len(entries) and \
            root_off + 2 * w <= nroots
        if ok:
            mine = entries[entry_off:entry_off + nshares]
            ok = all(pos < w and node_off + nnodes <= nnodes_total for pos, node_off, nnodes in mine) and \
                all(a[0] < b[0] for a, b in zip(mine, mine[1:]))
        pre = MALFORMED if not ok else TOO_FEW if nshares < k else 2
        lines.append(f"P {pre} {index if pre == 2 else 0}")
        if pre != 2:
            lines += [empty[0] + " 1"] * w
            continue
        mask = [0] * w
        for pos, _, _ in mine:
            mask[pos] = 1
        for j in range(w):
            if j >= nshares:
                lines.append(f"{empty[0]} {mask[j]}")
                continue
            pos, node_off, nnodes = mine[j]
            e = entry_off + j
            ns = bytes(shares[e][:NS]) if index < k and pos < k else b"\xff" * NS
            root = root_off + (w + pos if axis == 0 else pos)
            lines.append(f"{index} {index + 1} {node_off} {nnodes} {e} {root} {ns.hex()} {mask[j]}")
    return lines


def precheck_cases(k, seed):
    """One call's arrays: valid descriptors of every shape, and one of each way of being wrong, offsets outside the
    totals and counts near 2^32 among them."""
    rng = np.random.default_rng(seed)
    w, nblocks, nnodes_total = 2 * k, 3, 1000
    descs, entries = [], []
    for _ in range(24):
        n = int(rng.integers(0, w + 1))
        axis, index = int(rng.integers(0, 2)), int(rng.integers(0, w))
        descs.append([axis, index, len(entries), n, 2 * w * int(rng.integers(0, nblocks))])
        for pos in sorted(int(x) for x in rng.choice(w, n, replace=False)):
            nn = int(rng.integers(0, 12))
            entries.append([pos, int(rng.integers(0, nnodes_total - nn + 1)), nn])
    # runs of entries for the descriptors below: one in order, and one copy per way of breaking a run
    M, nroots = 0xFFFFFFFF, 2 * w * nblocks
    good = len(entries)
    entries += [[p, 7 * p, 3] for p in range(w)]
    broken = []
    for mutate in ("dup", "swap", "pos", "nodes", "nodes32"):
        run = [[p, 0, 1] for p in range(w)]
        if mutate == "dup":
            run[1][0] = run[0][0]
        elif mutate == "swap":
            run[0][0], run[1][0] = run[1][0], run[0][0]
        elif mutate == "pos":
            run[w - 1][0] = w
        elif mutate == "nodes":
            run[1][1:] = [nnodes_total - 1, 2]
        else:
            run[1][1:] = [M, 2]
        broken.append(len(entries))
        entries += run
    nentries = len(entries)
    descs += [[0, 0, good, w, 0], [1, w - 1, good, k, 2 * w * (nblocks - 1)],      # valid, at the last block
              [2, 0, good, w, 0], [M, 0, good, w, 0], [0, w, good, w, 0], [0, M, good, w, 0],
              [0, 0, good, w + 1, 0], [0, 0, good, M, 0], [0, 0, good, M - good + 1, 0],
              [0, 0, nentries - k + 1, k, 0], [0, 0, nentries, 1, 0], [0, 0, M, 2, 0], [0, 0, M - 1, 1, 0],
              [0, 0, good, w, nroots - 2 * w + 1], [0, 0, good, w, M], [0, 0, good, w, M - 2 * w + 1],
              [0, 0, good, k - 1, 0], [0, 0, nentries, 0, 0]]
    descs += [[0, 0, at, w, 0] for at in broken]
    shares = rng.integers(0, 256, (len(entries), N.SHARE_SIZE), dtype=np.uint8)
    return descs, entries, shares, nnodes_total, nroots


@pytest.fixture(scope="module")
def rule_dump(tmp_path_factory):
    """tests/san/befp_rule_dump.cpp + csrc/plan.cpp as a stand-alone executable under ASan and UBSan."""
    d = tmp_path_factory.mktemp("befp")
    exe = str(d / "befp_rule_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "befp_rule_dump.cpp"), os.path.join(CSRC, "plan.cpp")])

    def run(k, descs, entries, shares, nnodes_total, nroots):
        path = str(d / f"case_{k}.txt")
        with open(path, "w") as f:
            f.write(f"{k} {len(descs)} {len(entries)} {nnodes_total} {nroots}\n")
            f.writelines(" ".join(str(x) for x in r) + "\n" for r in descs)
            f.writelines(" ".join(str(x) for x in e) + " " + bytes(s).hex() + "\n" for e, s in zip(entries, shares))
        out = subprocess.run([exe, path], text=True, capture_output=True)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_cpp_precheck_matches_the_rule(rule_dump, k):
    case = precheck_cases(k, 0xBEF0 + k)
    want = precheck_mirror(k, *case)
    got = rule_dump(k, *case)
    assert got == want
    pres = {line.split()[1] for line in want if line.startswith("P ")}
    assert pres == {"2", str(MALFORMED), str(TOO_FEW)}


def test_precheck_mirror_is_validate_host():
    """The restatement above and validate_host reject the same proofs for the same reason (B1, B2)."""
    k = 2
    sq = HostSquare(honest_eds(k, 0xBE40), k)
    base = sq.create(1, 3)
    for shares in (base.shares, base.shares[:1], base.shares[::-1], base.shares[:2] + base.shares[1:],
                   [(4,) + base.shares[0][1:]] + base.shares[1:]):
        p = BadEncodingProof(1, 3, list(shares))
        descs, entries, cells, nodes = befp.pack([p], k)
        pre = precheck_mirror(k, descs.tolist(), entries.tolist(), cells, len(nodes), 4 * k)[0].split()[1]
        v = befp.validate_host(p, *sq.roots, codec=CODECS["leopard"])
        assert (v if v < 0 else 2) == int(pre)


# ---- the C ABI without a GPU ----
def test_entry_points_reject_a_null_context():
    L = N.lib()
    assert L.cda_square_open_eds(None, 4, None, None, None, None, None, None) == N.E_ARG
    assert L.cda_befp_validate(None, 4, 1, None, None, 0, None, None, 0, None, 0, None) == N.E_ARG
    assert L.cda_befp_validate_device(None, 4, 1, None, None, 0, None, None, 0, None, 0, None, None) == N.E_ARG


def test_bindings_match_the_header_records():
    import ctypes
    assert ctypes.sizeof(N.BefpDesc) == N.BEFP_DESC_DTYPE.itemsize == 20
    assert ctypes.sizeof(N.BefpEntry) == N.BEFP_ENTRY_DTYPE.itemsize == 12
    src = open(os.path.join(ROOT, "include", "cda.h")).read()
    for name in ("FRAUD", "NO_FRAUD", "MALFORMED", "TOO_FEW", "BAD_SHARE"):
        assert f"#define CDA_BEFP_{name} {getattr(N, 'BEFP_' + name)} " in src
