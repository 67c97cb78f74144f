"""What tests/test_codec_shapes.py (CPU) and tests/test_codec_shapes_gpu.py share: one case per launch shape of the
erasure decoder (csrc/rs_decode.hip) and of the GF(2^8) LDS encoder (rs_encode8_kernel, csrc/rs_kernels.hip), each
with the cell it claims to reach, and the presence masks the decoder cases use.

A cell is what decides which code a kernel runs (csrc/codec_shape.h has the rule, tests/san/codec_shape_dump.cpp
prints it).  The tables are literal on purpose: the CPU test asks the dump for every case's cell and for the set of all
reachable cells, so a retuned launch rule fails there until the tables follow it.
  decoder  (PL, log2 n, U, k < m)            PL bit planes (8: GF(2^8), 16: GF(2^16)), n = 2m, m = ceilPow2(k)
  encoder  (log2 m, U, lat, items > 512)     lat: the latency form; items = m * U > 512: the second load loop
"""
import numpy as np

# ---- decoder: one codeword through cda_rs_decode, the shard length alone selects U ----
# GF(2^8): L = 16 KiB * U for U > 1 (a unit is 32 bytes and the launch wants 512 workgroups); GF(2^16): 64 KiB for
# U = 2 (units of 64 bytes).  U = 1: 192 bytes, six / three units, so more than one workgroup and no power of two.
# k: the power of two and the smallest k above the previous one (k < m) of every n.
# patterns: "random_k" (exactly k survivors) and one more, cycling with the cell's index through PATTERNS so that every
# pattern meets every U of either field (test_codec_shapes.py checks that); GF(2^16) has too few cells for that and
# carries the missing ones as extra masks.  k = 1 has only the two masks with one survivor.
PATTERNS = ("parity_only", "data_only_minus_one", "window", "even", "ends", "random_k_plus_third")

DECODE_CASES = [
    # (k, L, (PL, log2n, U, k<m), patterns)
    (1, 192, (8, 1, 1, 0), ("data_only", "parity_only")),
    (1, 32768, (8, 1, 2, 0), ("data_only", "parity_only")),
    (1, 65536, (8, 1, 4, 0), ("data_only", "parity_only")),
    (1, 131072, (8, 1, 8, 0), ("data_only", "parity_only")),
    (1, 262144, (8, 1, 16, 0), ("data_only", "parity_only")),
    (2, 192, (8, 2, 1, 0), ("random_k", "parity_only")),
    (2, 32768, (8, 2, 2, 0), ("random_k", "data_only_minus_one")),
    (2, 65536, (8, 2, 4, 0), ("random_k", "window")),
    (2, 131072, (8, 2, 8, 0), ("random_k", "even")),
    (2, 262144, (8, 2, 16, 0), ("random_k", "ends")),
    (3, 192, (8, 3, 1, 1), ("random_k", "random_k_plus_third")),
    (3, 32768, (8, 3, 2, 1), ("random_k", "parity_only")),
    (3, 65536, (8, 3, 4, 1), ("random_k", "data_only_minus_one")),
    (3, 131072, (8, 3, 8, 1), ("random_k", "window")),
    (3, 262144, (8, 3, 16, 1), ("random_k", "even")),
    (4, 192, (8, 3, 1, 0), ("random_k", "ends")),
    (4, 32768, (8, 3, 2, 0), ("random_k", "random_k_plus_third")),
    (4, 65536, (8, 3, 4, 0), ("random_k", "parity_only")),
    (4, 131072, (8, 3, 8, 0), ("random_k", "data_only_minus_one")),
    (4, 262144, (8, 3, 16, 0), ("random_k", "window")),
    (5, 192, (8, 4, 1, 1), ("random_k", "even")),
    (5, 32768, (8, 4, 2, 1), ("random_k", "ends")),
    (5, 65536, (8, 4, 4, 1), ("random_k", "random_k_plus_third")),
    (5, 131072, (8, 4, 8, 1), ("random_k", "parity_only")),
    (5, 262144, (8, 4, 16, 1), ("random_k", "data_only_minus_one")),
    (8, 192, (8, 4, 1, 0), ("random_k", "window")),
    (8, 32768, (8, 4, 2, 0), ("random_k", "even")),
    (8, 65536, (8, 4, 4, 0), ("random_k", "ends")),
    (8, 131072, (8, 4, 8, 0), ("random_k", "random_k_plus_third")),
    (8, 262144, (8, 4, 16, 0), ("random_k", "parity_only")),
    (9, 192, (8, 5, 1, 1), ("random_k", "data_only_minus_one")),
    (9, 32768, (8, 5, 2, 1), ("random_k", "window")),
    (9, 65536, (8, 5, 4, 1), ("random_k", "even")),
    (9, 131072, (8, 5, 8, 1), ("random_k", "ends")),
    (9, 262144, (8, 5, 16, 1), ("random_k", "random_k_plus_third")),
    (16, 192, (8, 5, 1, 0), ("random_k", "parity_only")),
    (16, 32768, (8, 5, 2, 0), ("random_k", "data_only_minus_one")),
    (16, 65536, (8, 5, 4, 0), ("random_k", "window")),
    (16, 131072, (8, 5, 8, 0), ("random_k", "even")),
    (16, 262144, (8, 5, 16, 0), ("random_k", "ends")),
    (17, 192, (8, 6, 1, 1), ("random_k", "random_k_plus_third")),
    (17, 32768, (8, 6, 2, 1), ("random_k", "parity_only")),
    (17, 65536, (8, 6, 4, 1), ("random_k", "data_only_minus_one")),
    (17, 131072, (8, 6, 8, 1), ("random_k", "window")),
    (17, 262144, (8, 6, 16, 1), ("random_k", "even")),
    (32, 192, (8, 6, 1, 0), ("random_k", "ends")),
    (32, 32768, (8, 6, 2, 0), ("random_k", "random_k_plus_third")),
    (32, 65536, (8, 6, 4, 0), ("random_k", "parity_only")),
    (32, 131072, (8, 6, 8, 0), ("random_k", "data_only_minus_one")),
    (32, 262144, (8, 6, 16, 0), ("random_k", "window")),
    (33, 192, (8, 7, 1, 1), ("random_k", "even")),
    (33, 32768, (8, 7, 2, 1), ("random_k", "ends")),
    (33, 65536, (8, 7, 4, 1), ("random_k", "random_k_plus_third")),
    (33, 131072, (8, 7, 8, 1), ("random_k", "parity_only")),
    (64, 192, (8, 7, 1, 0), ("random_k", "data_only_minus_one")),
    (64, 32768, (8, 7, 2, 0), ("random_k", "window")),
    (64, 65536, (8, 7, 4, 0), ("random_k", "even")),
    (64, 131072, (8, 7, 8, 0), ("random_k", "ends")),
    (65, 192, (8, 8, 1, 1), ("random_k", "random_k_plus_third")),
    (65, 32768, (8, 8, 2, 1), ("random_k", "parity_only")),
    (65, 65536, (8, 8, 4, 1), ("random_k", "data_only_minus_one")),
    (128, 192, (8, 8, 1, 0), ("random_k", "window")),
    (128, 32768, (8, 8, 2, 0), ("random_k", "even")),
    (128, 65536, (8, 8, 4, 0), ("random_k", "ends")),
    (129, 192, (16, 9, 1, 1), ("random_k", "random_k_plus_third", "parity_only", "window")),
    (129, 65536, (16, 9, 2, 1), ("random_k", "parity_only", "even", "ends")),
    (256, 192, (16, 9, 1, 0), ("random_k", "data_only_minus_one")),
    (256, 65536, (16, 9, 2, 0), ("random_k", "window", "data_only_minus_one", "random_k_plus_third")),
    (257, 192, (16, 10, 1, 1), ("random_k", "even")),
    (512, 192, (16, 10, 1, 0), ("random_k", "ends")),
]

# 512 second-side halves at k = 16 through cda_axis_halves_verify: 512 codewords of 512-byte shards in one launch,
# offsets and strides from the prep kernel
HALVES_CASE = (16, 512, 512, (8, 5, 16, 0))  # (k, L, ncw, decoder cell)


def survivors(k, pattern, seed):
    """The presence mask (2k,) of a named loss pattern; at least k survive."""
    pres = np.zeros(2 * k, np.uint8)
    rng = np.random.default_rng(seed)
    if pattern == "random_k":
        pres[rng.choice(2 * k, k, replace=False)] = 1
    elif pattern == "random_k_plus_third":
        pres[rng.choice(2 * k, k + k // 3, replace=False)] = 1
    elif pattern == "data_only":
        pres[:k] = 1
    elif pattern == "parity_only":
        pres[k:] = 1
    elif pattern == "data_only_minus_one":  # one data shard lost, everything else present
        pres[:] = 1
        pres[int(rng.integers(0, k))] = 0
    elif pattern == "window":
        pres[k // 2:k // 2 + k] = 1
    elif pattern == "even":
        pres[0::2] = 1
    elif pattern == "ends":  # the first ceil(k/2) data shards and the last floor(k/2) parity shards
        pres[:(k + 1) // 2] = 1
        pres[2 * k - k // 2:] = 1
    else:
        raise ValueError(pattern)
    assert pres.sum() >= k and (pattern in ("random_k_plus_third", "data_only_minus_one") or pres.sum() == k)
    return pres


# ---- GF(2^8) LDS encoder ----
# form "host": one codeword through cda_rs_encode; "device": ncw codewords through cda_rs_encode_device in both layouts.
# At k >= 16 the LDS encoder takes what the register encoder does not: an odd k, an odd number of codewords or a
# shard length that is no multiple of 512, and (the latency form) launches that would leave most of the chip idle.
# A power-of-two k and a k < m for every cell with log2 m >= 2: the cell and (k < m) together are a case's key.
ENCODE8_CASES = [
    # (k, L, ncw, form, (log2m, U, lat, items>512))
    (1, 64, 1, "host", (0, 2, 0, 0)),
    (1, 128, 1, "host", (0, 4, 0, 0)),
    (1, 256, 1, "host", (0, 8, 0, 0)),
    (1, 512, 1, "host", (0, 16, 0, 0)),
    (2, 64, 1, "host", (1, 2, 0, 0)),
    (2, 128, 1, "host", (1, 4, 0, 0)),
    (2, 256, 1, "host", (1, 8, 0, 0)),
    (2, 512, 1, "host", (1, 16, 0, 0)),
    (3, 64, 1, "host", (2, 2, 0, 0)),
    (3, 128, 1, "host", (2, 4, 0, 0)),
    (3, 256, 1, "host", (2, 8, 0, 0)),
    (3, 512, 1, "host", (2, 16, 0, 0)),
    (4, 64, 1, "host", (2, 2, 0, 0)),
    (4, 128, 1, "host", (2, 4, 0, 0)),
    (4, 256, 1, "host", (2, 8, 0, 0)),
    (4, 512, 1, "host", (2, 16, 0, 0)),
    (5, 64, 1, "host", (3, 2, 0, 0)),
    (5, 128, 1, "host", (3, 4, 0, 0)),
    (5, 256, 1, "host", (3, 8, 0, 0)),
    (5, 512, 1, "host", (3, 16, 0, 0)),
    (8, 64, 1, "host", (3, 2, 0, 0)),
    (8, 128, 1, "host", (3, 4, 0, 0)),
    (8, 256, 1, "host", (3, 8, 0, 0)),
    (8, 512, 1, "host", (3, 16, 0, 0)),
    (9, 64, 3, "device", (4, 2, 0, 0)),
    (9, 128, 3, "device", (4, 4, 1, 0)),
    (9, 512, 64, "device", (4, 16, 0, 0)),
    (9, 640, 64, "device", (4, 4, 0, 0)),
    (9, 768, 65, "device", (4, 8, 0, 0)),
    (16, 64, 3, "device", (4, 2, 0, 0)),
    (16, 128, 3, "device", (4, 4, 1, 0)),
    (16, 512, 65, "device", (4, 16, 0, 0)),
    (16, 640, 64, "device", (4, 4, 0, 0)),
    (16, 768, 65, "device", (4, 8, 0, 0)),
    (17, 64, 3, "device", (5, 2, 0, 0)),
    (17, 128, 3, "device", (5, 4, 1, 0)),
    (17, 512, 64, "device", (5, 16, 0, 0)),
    (17, 640, 64, "device", (5, 4, 0, 0)),
    (17, 768, 65, "device", (5, 8, 0, 0)),
    (32, 64, 3, "device", (5, 2, 0, 0)),
    (32, 128, 3, "device", (5, 4, 1, 0)),
    (32, 512, 65, "device", (5, 16, 0, 0)),
    (32, 640, 64, "device", (5, 4, 0, 0)),
    (32, 768, 65, "device", (5, 8, 0, 0)),
    (33, 64, 3, "device", (6, 2, 0, 0)),
    (33, 128, 3, "device", (6, 4, 1, 0)),
    (33, 512, 64, "device", (6, 16, 0, 1)),
    (33, 640, 64, "device", (6, 4, 0, 0)),
    (33, 768, 65, "device", (6, 8, 0, 0)),
    (64, 64, 3, "device", (6, 2, 0, 0)),
    (64, 128, 3, "device", (6, 4, 1, 0)),
    (64, 512, 65, "device", (6, 16, 0, 1)),
    (64, 640, 64, "device", (6, 4, 0, 0)),
    (64, 768, 65, "device", (6, 8, 0, 0)),
    (65, 64, 3, "device", (7, 2, 0, 0)),
    (65, 128, 3, "device", (7, 4, 1, 0)),
    (65, 512, 64, "device", (7, 16, 0, 1)),
    (65, 640, 64, "device", (7, 4, 0, 0)),
    (65, 768, 65, "device", (7, 8, 0, 1)),
    (128, 64, 3, "device", (7, 2, 0, 0)),
    (128, 128, 3, "device", (7, 4, 1, 0)),
    (128, 512, 65, "device", (7, 16, 0, 1)),
    (128, 640, 64, "device", (7, 4, 0, 0)),
    (128, 768, 65, "device", (7, 8, 0, 1)),
]


def ceil_pow2(k):
    m = 1
    while m < k:
        m *= 2
    return m


def encode8_key(k, cell):
    """What one encoder case stands for: its cell and, where m has room for it (log2 m >= 2), whether k < m."""
    return cell + ((int(k < ceil_pow2(k)),) if cell[0] >= 2 else ())
