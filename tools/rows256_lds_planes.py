#!/usr/bin/env python3
"""Host-side model of the per-wave exchange of gl::rows256_kernel (ntt_goldilocks.hpp: Wave256 / wave256_exchange).

A wave owns 1 088 32-bit words of LDS; word p (0..1023: the wave's four rows of 256) lives at p + (p >> 4).  Checked here:
  * the three access patterns are the ones the old workgroup-wide tile used (pad(rho 256 + i0 + 16 s), 17 t + j, pad(j 256 + t)
    replaced by a per-wave coalesced order), restricted to a wave: every word a lane reads was written by a lane of the SAME wave;
  * each pattern is a bijection between (lane, register) and the wave's words, inside the region;
  * bank conflicts of ds_write_b32 / ds_read_b32 (MI355X: 32 lanes per LDS cycle, bank = word address mod 32).
"""
WORDS = 1024 + 64


def pad(p):
    return p + (p >> 4)


def strided(l, s):   # lane (r, i0) of the wave, register s: coefficient i0 + 16 s of row r
    return 272 * (l >> 4) + (l & 15) + 17 * s


def own(l, j):       # the lane's 16 consecutive slots
    return 17 * l + j


def coalesced(l, j):  # tile position 1 024 w + 64 j + l
    return l + (l >> 4) + 68 * j


def worst_conflict(pattern):
    worst = 1
    for k in range(16):
        for g in (0, 32):
            banks = {}
            for l in range(g, g + 32):
                banks.setdefault(pattern(l, k) % 32, set()).add(pattern(l, k))
            worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def main():
    # the patterns are the padded positions of the words they claim to be
    for l in range(64):
        for k in range(16):
            assert strided(l, k) == pad(256 * (l >> 4) + (l & 15) + 16 * k)
            assert own(l, k) == pad(16 * l + k)
            assert coalesced(l, k) == pad(64 * k + l)
    for name, pat in (("strided", strided), ("own", own), ("coalesced", coalesced)):
        cells = sorted(pat(l, k) for l in range(64) for k in range(16))
        assert cells == sorted(pad(p) for p in range(1024)) and cells[-1] < WORDS, name
        print("%-9s bijection onto the wave's 1024 words, max word %d of %d, worst bank conflict %d-way" % (name, cells[-1], WORDS, worst_conflict(pat)))
    assert worst_conflict(strided) == 1 and worst_conflict(own) == 1 and worst_conflict(coalesced) == 2
    # wave-locality in the old workgroup-wide index space: lane t = 64 w + l writes pad(rho 256 + i0 + 16 s), reads 17 t + j
    for t in range(256):
        w = t >> 6
        for k in range(16):
            wrote = (t >> 4) * 256 + (t & 15) + 16 * k
            read = 16 * t + k
            assert wrote >> 10 == w and read >> 10 == w  # both inside the wave's own 1 024 positions
            assert strided(t & 63, k) == pad(wrote - 1024 * w) and own(t & 63, k) == pad(read - 1024 * w)
    # the exchange is the 16 x 16 transpose of each row: what lane (r, i0) wrote from register s, lane (r, s) reads into register i0
    for l in range(64):
        for s in range(16):
            assert strided(l, s) == own((l & 48) | s, l & 15)
    print("rows256 per-wave exchange: wave-local, conflict-free for the fused products")


if __name__ == "__main__":
    main()
