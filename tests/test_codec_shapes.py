"""CPU tests of the codec launch rules (csrc/codec_shape.h): which shape launch_rs_decode and launch_rs_encode8 give a
(k, shard length, number of codewords), asked of tests/san/codec_shape_dump.cpp, a stand-alone host program built and
run under ASan + UBSan.  They pin that the cases of tests/codec_cases.py (run on the device by
tests/test_codec_shapes_gpu.py) reach every shape the rules can produce: a retuned rule, or a deleted case, fails here
and names the cell that no case reaches any more."""
import os
import subprocess

import pytest

import codec_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC_MAX_LDS, ENC8_MAX_LDS = 144 * 1024, 128 * 1024  # the kernels' hipFuncSetAttribute caps


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("codec_shape") / "codec_shape_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "san", "codec_shape_dump.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")

    def run(args=(), stdin=""):
        out = subprocess.run([exe, *args], input=stdin, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        return out.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def cells(dump):
    """The walk of the whole domain: (decoder cells, encoder cells, violations, (shapes walked))."""
    dec, enc, bad, checked = {}, {}, [], None
    for line in dump(["cells"]):
        f = line.split()
        if f[0] in "DE":
            assert f[5] == ":"
            (dec if f[0] == "D" else enc)[tuple(int(x) for x in f[1:5])] = tuple(int(x) for x in f[6:9])
        elif f[0] == "V":
            bad.append(line)
        else:
            assert f[0] == "checked" and checked is None
            checked = (int(f[1]), int(f[2]))
    return dec, enc, bad, checked


def ask(dump, lines):
    """One answer per question, the question stripped: a tuple of fields, or None for "unsupported"."""
    got = dump(stdin="".join(q + "\n" for q in lines))
    assert len(got) == len(lines)
    out = []
    for q, a in zip(lines, got):
        head, answer = a.split(" : ")
        assert head == q
        out.append(None if answer == "unsupported" else tuple(answer.split()))
    return out


def dec_cell(k, answer):
    PL, m, n, log2n, U, slices, lds = (int(x) for x in answer)
    return (PL, log2n, U, int(k < m))


def test_whole_domain_meets_the_kernels_preconditions(cells):
    """Over k = 1..512 (decoder) and 1..128 (encoder) at every shard length and batch size of the walk: a shape is
    given, n * U <= 1024, U * slices * unit == shard_len and the LDS fits the cap (the program prints each miss)."""
    dec, enc, bad, checked = cells
    assert bad == []
    assert checked == (512 * (32 + 510) * 8, 128 * 64 * 7)
    # the same of the cells themselves: n * U and the LDS bytes are functions of the cell
    for PL, log2n, U, _ in dec:
        n = 1 << log2n
        assert n * U <= 1024, (PL, log2n, U)  # raw[4] and nv[4]: four items per thread at 256 threads
        assert n * PL * U * 4 + n * 8 <= DEC_MAX_LDS
        assert PL == (8 if n <= 256 else 16)
    for log2m, U, lat, second in enc:
        items = (1 << log2m) * U
        assert second == int(items > 512)
        assert items * 8 * 4 + (2048 if lat else 0) <= ENC8_MAX_LDS
        assert not lat or log2m >= 4


def test_the_walk_finds_the_expected_number_of_cells(cells):
    dec, enc, _, _ = cells
    assert (len(dec), len(enc)) == (70, 36)
    # GF(2^8): U <= min(16, 1024 / n); GF(2^16): n = 512 with U in {1, 2}, n = 1024 with U = 1; k < m needs m >= 4
    want = {(8 if n <= 256 else 16, n.bit_length() - 1, U, lt)
            for n in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) for U in (1, 2, 4, 8, 16) for lt in (0, 1)
            if n * U <= 1024 and (n <= 256 or U <= 2) and (not lt or n >= 8)}
    assert set(dec) == want


def test_every_decode_case_reaches_the_cell_beside_it_and_all_cells_are_reached(dump, cells):
    cases = CC.DECODE_CASES
    got = ask(dump, [f"dec {k} {L} 1" for k, L, _, _ in cases])
    for (k, L, cell, _), a in zip(cases, got):
        assert a is not None and dec_cell(k, a) == cell, (k, L)
        PL, m, n, log2n, U, slices, lds = (int(x) for x in a)
        assert U * slices * PL * 4 == L and n * U <= 1024 and lds <= DEC_MAX_LDS
        assert slices > 1 or U == 1  # one codeword: the launch is split over workgroups wherever U > 1
    hit = [cell for _, _, cell, _ in cases]
    assert len(set(hit)) == len(hit), "two cases claim one cell"
    missing = set(cells[0]) - set(hit)
    assert not missing, f"decoder cells (PL, log2n, U, k<m) that no case reaches: {sorted(missing)}"
    assert set(hit) == set(cells[0])
    # the batched case: many codewords of 512-byte shards
    k, L, ncw, cell = CC.HALVES_CASE
    (a,) = ask(dump, [f"dec {k} {L} {ncw}"])
    assert dec_cell(k, a) == cell and int(a[5]) == 1  # one workgroup per codeword


def test_every_pattern_meets_every_u_of_each_field():
    for k, L, cell, patterns in CC.DECODE_CASES:
        assert len(patterns) >= 2 and len(set(patterns)) == len(patterns)
        if k == 1:
            assert set(patterns) == {"data_only", "parity_only"}  # the two masks with one survivor
        else:
            assert patterns[0] == "random_k" and set(patterns[1:]) <= set(CC.PATTERNS)
        for p in patterns:
            pres = CC.survivors(k, p, 1)
            want = {"random_k_plus_third": k + k // 3, "data_only_minus_one": 2 * k - 1}.get(p, k)
            assert pres.shape == (2 * k,) and int(pres.sum()) == want
            if p == "data_only_minus_one":
                assert pres[k:].all()
    for PL, U in {(c[0], c[2]) for _, _, c, _ in CC.DECODE_CASES}:
        seen = {p for k, _, c, ps in CC.DECODE_CASES if (c[0], c[2]) == (PL, U) and k > 1 for p in ps}
        assert seen == {"random_k", *CC.PATTERNS}, (PL, U)


def test_every_encode_case_reaches_the_cell_beside_it_and_all_cells_are_reached(dump, cells):
    cases = CC.ENCODE8_CASES
    got = ask(dump, [f"enc8 {k} {L} {ncw}" for k, L, ncw, _, _ in cases])
    for (k, L, ncw, form, cell), a in zip(cases, got):
        assert a is not None and a[0] == "lds", (k, L, ncw, a)  # not the register encoder's
        log2m, U, slices, lat, lds = (int(x) for x in a[1:])
        assert (log2m, U, lat, int((1 << log2m) * U > 512)) == cell, (k, L, ncw)
        assert U * slices * 32 == L and lds <= ENC8_MAX_LDS
        assert form == ("host" if ncw == 1 else "device")
    keys = [CC.encode8_key(k, cell) for k, _, _, _, cell in cases]
    assert len(set(keys)) == len(keys), "two cases claim one cell and side of m"
    want = {cell + ((lt,) if cell[0] >= 2 else ()) for cell in cells[1] for lt in ((0, 1) if cell[0] >= 2 else (0,))}
    missing = want - set(keys)
    assert not missing, f"encoder cells (log2m, U, lat, items>512[, k<m]) that no case reaches: {sorted(missing)}"
    assert set(keys) == want


def test_unsupported_inputs_give_no_shape(dump):
    q = ["dec 513 512 1", "dec 1024 512 64", "dec 32768 64 1", "dec 32769 64 1", "dec 0 512 1", "dec 16 96 1",
         "dec 16 32 1", "dec 16 512 0", "enc8 129 512 1", "enc8 0 512 1", "enc8 4 96 1", "enc8 16 544 64",
         "enc8 16 512 0"]
    assert ask(dump, q) == [None] * len(q)
    # and their neighbours do
    ok = ask(dump, ["dec 512 512 1", "dec 16 64 1", "enc8 128 512 1", "enc8 4 64 1", "enc8 16 512 64"])
    assert None not in ok and ok[-1][0] == "reg"
