"""A numpy model of the privacy amplification hash in its matrix form, for the tests of
the long form (tests/test_privacy_long.py): out_i = parity of x & r[i : i + n_in]. A
helper of the tests, not part of the product."""
import numpy as np


def splitmix_words(seed, count):
    """R[k] = mix(seed + (k + 1) * golden) mod 2^64 (SplitMix64 in counter form)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key_words(n_in, L):
    return (n_in + L - 1 + 63) // 64


def key_bits(R, count):
    """Bits 0 .. count - 1 of the key string R (uint64 words), as uint8."""
    k = np.arange(count)
    return ((np.asarray(R, np.uint64)[k >> 6] >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def pack_bits(bits):
    """[F, L] 0/1 -> uint64 [F, ceil(L / 64)], bit i in word i >> 6 at i & 63."""
    f, L = bits.shape
    padded = np.zeros((f, (L + 63) // 64 * 64), np.uint64)
    padded[:, :L] = bits
    return np.bitwise_or.reduce(padded.reshape(f, -1, 64) << np.arange(64, dtype=np.uint64), axis=2)


def model_hash(R, keys, L):
    """A[i, p] = r[p + i] (L x n_in, Hankel), out = A x over GF(2), in row blocks of A
    (binary32 products are exact: the sums stay below 2^24). keys [F, n_in] bytes (a key
    bit is byte & 1) -> uint64 [F, ceil(L / 64)]."""
    x = (np.atleast_2d(keys) & 1).astype(np.float32)
    f, n = x.shape
    assert len(R) == key_words(n, L) and n < 2**24
    rows = np.lib.stride_tricks.sliding_window_view(key_bits(R, n + L - 1).astype(np.float32), n)
    assert rows.shape == (L, n)                                   # rows[i] = r[i : i + n]
    bits = np.zeros((f, L), np.uint64)
    step = max(1, (1 << 24) // n)
    for i0 in range(0, L, step):
        A = np.ascontiguousarray(rows[i0:i0 + step])
        bits[:, i0:i0 + A.shape[0]] = (x @ A.T).astype(np.int64) & 1
    return pack_bits(bits)
