#!/usr/bin/env python3
"""Bank conflicts of the TILE form's LDS layout (csrc/wave_files_kernels.hip), enumerated from the address arithmetic.

No GPU: this is the arithmetic of lds_at / lds_dword / Walk and the bank rule (a / 4) mod 32 within each 32-lane half
(ds_read_b32, ds_read_u16 / u8 taken as the same, every ds_write).  Lanes of one half that name the SAME dword broadcast
(reads) or merge (the two halves of a dword on the planar side) and count once.  The degree printed is the worst over every
half-wave of the 256 lanes, every round of a full span and every step; 1 means conflict-free.  DESIGN.md 4.6i carries the
table this prints.  It is a derivation, not a measurement: no SQ_LDS_BANK_CONFLICT run has been made.
"""
import sys

SPAN_BYTES, PAD, LANES = 16384, 4, 256


def lds_at(p, P):
    return p + PAD * (p // P)


def lds_dword(p, i, P):                        # dword i of the vector at position p = 16 v
    q, rem = divmod(p, P)
    return p + 4 * i + PAD * (q + (1 if rem + 4 * i >= P else 0))


def degree(addresses):                         # of one half-wave's byte addresses
    banks = {}
    for a in set(a // 4 for a in addresses):
        banks[a % 32] = banks.get(a % 32, 0) + 1
    return max(banks.values()) if banks else 1


def rotates(P):                                # the kernel's choice (interleaved_rot)
    return P > 256


def interleaved(P, span, rotate):
    worst = 1
    for first in range(0, span // 16, 32):     # half-waves: 32 consecutive vectors
        for k in range(4):
            adr = []
            for v in range(first, min(first + 32, span // 16)):
                lane = v % LANES
                i = (k + lane // 8) & 3 if rotate else k
                adr.append(lds_dword(16 * v, i, P))
            worst = max(worst, degree(adr))
    return worst


def planar(nch, bps, span, pad=True):
    frame = nch * bps
    P = 8 * frame
    groups = span // P
    worst = 1
    for first in range(0, groups * nch, 32):
        for j in range(8):
            adr = []
            for e in range(first, min(first + 32, groups * nch)):
                c, g = divmod(e, groups)
                p = (8 * g + j) * frame + c * bps
                adr.append(lds_at(p, P) if pad else p)
            worst = max(worst, degree(adr))
    return worst


def main():
    print("channels bits  P      planar: unpadded padded   interleaved: fixed dword  rotated  kernel")
    for bits in (16, 8):
        for nch in (1, 2, 6, 8, 33, 255):
            bps = bits // 8
            frame = nch * bps
            P = 8 * frame
            span = SPAN_BYTES // frame // 8 * 8 * frame
            fixed, rot = interleaved(P, span, False), interleaved(P, span, True)
            print(f"{nch:8d} {bits:4d} {P:5d} {planar(nch, bps, span, False):17d} {planar(nch, bps, span):6d}"
                  f" {fixed:25d} {rot:8d} {rot if rotates(P) else fixed:7d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
