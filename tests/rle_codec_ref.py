"""fs_rle_bits' definition in plain Python / numpy (include/fovealseg.h), beside tests/rle_ref.py, which it imports and does not change:
the decoder of the uncompressed run-length code with its info row, and the compressed string form written the other way round from
ops.rle_to_string / ops.rle_from_string (digit by digit, from the published definition of pycocotools' rleToString / rleFrString).
Unpinned like rle_ref: tests/test_rle_decode.py holds this file to hand-derived answers first."""
import numpy as np

import rle_ref as R

OK, CUT, BAD, SUM = 0, 1, 2, 3


def decode_info(counts_row, n_runs, Hs, Ws):
    """counts_row: the cap entries of one image's row (anything at or past n_runs is never looked at).  -> (mask (Hs,Ws) bool,
    [status, area, n_read, total]); the mask is all False where status is not 0."""
    cap, N = len(counts_row), Hs * Ws
    n_read = min(max(int(n_runs), 0), cap)
    read = [int(v) for v in counts_row[:n_read]]
    total = sum(read)
    if n_runs > cap:
        status = CUT
    elif n_runs < 1 or any(v < 0 for v in read):
        status = BAD
    elif total != N:
        status = SUM
    else:
        status = OK
    if status != OK:
        return np.zeros((Hs, Ws), dtype=bool), [status, 0, n_read, total]
    v = np.zeros(N, dtype=bool)
    p = 0
    for i, c in enumerate(read):                          # a zero-length run moves nothing
        if i & 1:
            v[p:p + c] = True
        p += c
    return v.reshape(Ws, Hs).T.copy(), [OK, sum(read[1::2]), n_read, total]


def with_zero_runs(code, rng, k=3):
    """The same mask written with k zero-length runs more: a count c becomes a, 0, c - a (a run entered, left at once and resumed); two
    of them also go in front ([0, 0] + code: an empty run of each kind) and two behind."""
    code = list(code)
    for _ in range(k):
        i = int(rng.integers(0, len(code)))
        a = int(rng.integers(0, code[i] + 1))
        code[i:i + 1] = [a, 0, code[i] - a]
    return [0, 0] + code + [0, 0]


def to_string(counts):
    """The compressed form, by digits: the difference to the count two back (from the fourth count on) in two's-complement base 32, low
    digit first, as few digits as keep the sign bit (16) of the last one right; every digit but the last plus 32; chr(digit + 48)."""
    s = ""
    for i, c in enumerate(counts):
        x = c - counts[i - 2] if i > 2 else c
        n = 1
        while not -(1 << (5 * n - 1)) <= x < (1 << (5 * n - 1)):
            n += 1
        y = x & ((1 << (5 * n)) - 1)                      # two's complement on 5 n bits
        for k in range(n):
            d = (y >> (5 * k)) & 31
            s += chr(d + (32 if k < n - 1 else 0) + 48)
    return s


def mask_of(code, Hs, Ws):
    return R.decode(code, Hs, Ws)
