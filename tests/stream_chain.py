"""A Python statement of the stream decoder's chain rule (steps B and C of sf_stream.hip, DESIGN.md 3a "Streams without flush
points"), over an abstract stream: the serial decoder's block sequence is a list of block ends (bit positions), and a decode
from a position that is not a block start either fails or runs into arbitrary "garbage" block ends.  TEST INFRASTRUCTURE ONLY."""
import bisect

import numpy as np


class Stream:
    def __init__(self, ends, rng, garbage_error=0.5):
        self.ends = ends  # block k covers [ends[k-1], ends[k]); ends[-1] is the final block's end; block 0 starts at 0
        self.starts = [0] + ends[:-1]
        self.rng = rng
        self.garbage_error = garbage_error
        self.fake = {}

    def decode(self, start, limit):
        """blocks from `start` until the first block end >= limit, or the final block -> (end, final, status, blocks)"""
        if start >= limit:
            return start, False, 0, []
        k = bisect.bisect_left(self.starts, start)
        if k < len(self.starts) and self.starts[k] == start:
            blocks = []
            while True:
                blocks.append(k)
                end = self.ends[k]
                if k == len(self.ends) - 1:
                    return end, True, 0, blocks
                if end >= limit:
                    return end, False, 0, blocks
                k += 1
        # a false start: a fixed (per position) outcome -- an error, or a fake run of blocks that ends somewhere
        if start not in self.fake:
            if limit == float("inf") or self.rng.random() < self.garbage_error:  # (the last chunk runs until it fails)
                self.fake[start] = None
            else:
                self.fake[start] = start + 1 + int(self.rng.integers(0, 4 * (limit - start) + 8))
        e = self.fake[start]
        if e is None:
            return start, False, 1, ["garbage"]
        if e < limit:  # keeps going: the fake blocks end past the limit eventually
            e = limit + (e % 7)
        return e, False, 0, ["garbage"]


INF = (1 << 64) - 1


def chain(stream, candidates, round_fn=None):
    """candidates: sorted bit positions (0 first) -> (the blocks of the confirmed chain, its last record, rounds).  round_fn:
    step C on a stream_host.CHUNK array, in place -> (redo, confirmed) -- stream_host.chain_round runs the library's own
    sf::stream_chain_round.  A repair round decodes the redo chunks, then, as k_stream_decode's follow launch does, the first
    of them goes on into the chunks after it while their links break."""
    import stream_host as H

    round_fn = round_fn or H.chain_round
    m = len(candidates)
    rec = np.zeros(m, H.CHUNK)
    rec["start"] = candidates
    rec["limit"][:-1] = candidates[1:]
    rec["limit"][-1] = INF
    blocks = [None] * m

    def run(i):
        lim = float("inf") if rec["limit"][i] == INF else int(rec["limit"][i])
        end, fin, st, blocks[i] = stream.decode(int(rec["start"][i]), lim)
        rec["end"][i], rec["final"][i], rec["status"][i] = end, int(fin), st

    for i in range(m):
        run(i)
    rounds = 0
    while True:
        before = rec["start"].copy()
        redo, confirmed = round_fn(rec)
        for i in np.nonzero(rec["start"] != before)[0]:  # moved and not decoded again: settled empty by step C
            if i not in redo:
                blocks[i] = []
        if not redo:
            break
        rounds += 1
        for i in redo:
            run(i)
        i, j = redo[0], redo[0] + 1  # (the follow launch: the first broken link goes on while links break)
        while j < m and not rec["status"][i] and not rec["final"][i] and rec["end"][i] != rec["start"][j]:
            rec["limit"][i] = rec["end"][i]
            rec["start"][j] = rec["end"][i]
            run(j)
            i, j = j, j + 1
    out = [b for k in range(confirmed) for b in blocks[k]]
    last = {"final": bool(rec["final"][confirmed - 1]), "status": int(rec["status"][confirmed - 1])}
    return out, last, rounds
