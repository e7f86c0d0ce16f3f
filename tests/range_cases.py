"""Ranges for the random-access tests: the edge cases of a stream's segment and strip geometry plus seeded random ones."""
import numpy as np

SEG = 32768


def edge_ranges(total_n, block_bytes):
    """(offset, length) pairs that start or end on segment and strip edges, one byte either side of them, in the last
    partial segment, of zero length, and covering the whole stream."""
    strip = block_bytes or SEG
    out = [(0, total_n), (0, 0), (total_n, 0), (total_n // 2, 0)]
    if total_n == 0:
        return out
    marks = set()
    for edge in (SEG, 2 * SEG, strip, 2 * strip, strip + SEG, (total_n // SEG) * SEG, (total_n // strip) * strip, total_n):
        for d in (-1, 0, 1):
            if 0 <= edge + d <= total_n:
                marks.add(edge + d)
    marks = sorted(marks)
    for a in marks:
        for ln in (1, 2, 5, SEG - 1, SEG, SEG + 1, strip, strip + 1):
            if a + ln <= total_n:
                out.append((a, ln))
        for b in marks:
            if a < b and b - a <= 2 * strip + 2 * SEG:
                out.append((a, b - a))
    last = (total_n - 1) // SEG * SEG  # the last (maybe partial) segment
    out += [(last, total_n - last), (min(last + 1, total_n - 1), 1), (total_n - 1, 1)]
    if total_n - last > 2:
        out.append((last + 1, total_n - last - 2))
    return sorted(set(out))


def random_ranges(rng, total_n, n, max_len=3 * SEG):
    out = []
    for _ in range(n if total_n else 0):
        ln = int(rng.integers(0, min(max_len, total_n) + 1))
        if rng.integers(0, 4) == 0:
            ln = int(rng.integers(0, min(300, total_n) + 1))
        out.append((int(rng.integers(0, total_n - ln + 1)), ln))
    return out
