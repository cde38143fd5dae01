#!/usr/bin/env python3
"""Per-frame instruction budget of gc_encode_persistent_kernel<8, false> from hipcc's ISA listing: where do
the ~409 lane-operations per input sample go against the ~240 the two passes x 8 predictors need?

The frame loop's basic blocks are found from the listing itself: the seven `v_dot2_i32_i16 v, E, E, acc clamp` of a quantise pass
(gc_encode_core.hpp E3: total += e0 * e0 + e1 * e1, once per two sample steps since round 8) mark the passes; the blocks between the loop's labels are classified by what they hold.
Prints static instruction counts per block of the HOT path of one frame (lane = (channel, predictor), CPW = 8: one wave-frame
= 8 channel-frames = 112 samples), the cold block's path for a plain third trip, the helper wave's loop per tile, and the
resulting lane-operations per sample with the measured rates (cold-block rate, short-pass share) filled in.

    python tools/isa_budget_gc.py > profiles/rNN_gc_encode_isa_budget.md

(Tables up to profiles/r08_gc_encode_isa_budget.md were made with an earlier frame-start rule that counted the tile head into
the frame's first row -- 87 VALU where this version says 53 for the same source; they cannot be reproduced with this version.)
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vgaudio_amd", "csrc", "gc_encode_kernel.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fwrapv", "-fno-fast-math", "-w"]
COLD_RATE = 0.3445          # bench.py signal_sensitivity, synthetic: cold blocks per wave-frame (profiles/r06 bench line)
SHORT_SHARE = 0.70          # wave-frames whose two passes run without the f32 detour (LABNOTES 9.7)


def listing():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["--save-temps=obj", "-c", SRC, "-o", os.path.join(tmp, "k.o")], check=True, cwd=tmp,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f][0]
        return open(os.path.join(tmp, s)).read().split("\n")


def kernel(lines, name):
    a = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l and l.split(";")[0].rstrip().endswith(":"))
    b = next(i for i in range(a, len(lines)) if "s_endpgm" in lines[i])
    out = []
    for l in lines[a + 1:b + 1]:
        t = l.split(";")[0].rstrip()
        if not t.strip() or t.strip().startswith((".p2align", ".", "//")) and not t.strip().endswith(":"):
            continue
        out.append(t.strip())
    return out


def count(block):
    c = collections.Counter()
    for t in block:
        if t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_"):
            c["VALU"] += 1
        elif op.startswith(("s_waitcnt", "s_nop")):
            c["wait/nop"] += 1
        elif op.startswith("s_"):
            c["SALU"] += 1
        elif op.startswith("ds_"):
            c["LDS"] += 1
        elif op.startswith(("global_", "scratch_", "buffer_", "flat_")):
            c["VMEM"] += 1
        else:
            c["other"] += 1
    c["total"] = sum(v for k, v in c.items() if k != "total")
    return c


def main():
    L = kernel(listing(), "gc_encode_persistent_kernelILi8ELb0E")
    sq = [i for i, l in enumerate(L) if re.search(r"v_dot2_i32_i16 v\d+, (v\d+), \1, (?:v\d+|0) clamp", l)]
    assert len(sq) >= 28, "the listing does not look like the encoder's"
    # first frame of the loop body (row set A): squares 0..27 = short pair (2 x 7) + normal pair (2 x 7)
    # (hipcc sinks the short pair's squares behind the passes, into a block of their own: the passes' extent is taken from
    # the fourteen v_cvt_pk_i16_i32 of each -- clamp and history shift, on the chain -- and stretched over the squares)
    cv = [i for i, l in enumerate(L) if l.startswith("v_cvt_pk_i16_i32") and i > sq[0] - 700]
    assert len(cv) >= 56, "the listing does not look like the encoder's"
    short_a, short_b = min(cv[0], sq[0]), max(cv[27], sq[13])
    normal_a, normal_b = min(cv[28], sq[14]), max(cv[55], sq[27])
    labels = [i for i, l in enumerate(L) if l.endswith(":")]
    prev_label = lambda i: max(j for j in labels if j <= i)
    next_label = lambda i: min(j for j in labels if j > i)
    # the frame's first label: the nearest one in front of the passes whose block opens with the row reads of the NEXT frame
    # (six ds_read_b128) -- the small blocks between it and the passes are the pre-scan head, the first scale and the
    # rare sequential pre-scan
    frame_start = max(j for j in labels if j < short_a and sum(l.startswith("ds_read_b128") for l in L[j:j + 20]) >= 6)
    short_blk = (prev_label(short_a), next_label(short_b))
    normal_blk = (prev_label(normal_a), next_label(normal_b))
    tail_end = normal_blk[1]
    while not L[tail_end].startswith("s_branch"):
        tail_end += 1
    # (what an execz branch jumps over -- the rare +M / -M tie's sequential pre-scan -- is not on the hot path)
    pre, skip_to = [], None
    for t in L[frame_start:short_blk[0]]:
        if skip_to:
            if t == skip_to + ":":
                skip_to = None
            continue
        pre.append(t)
        if t.startswith("s_cbranch_execz"):
            skip_to = t.split()[1]
    rows = [("row reads (6 x ds_read_b128) + pre-scan of the two history-dependent distances + first scale", count(pre)),
            ("passes B (s1 + 1) and A (s1) without the f32 detour, 28 sample steps", count(L[short_blk[0]:short_blk[1]])),
            ("the same with the conversions (30 % of the wave-frames take these instead)", count(L[normal_blk[0]:normal_blk[1]])),
            ("select the pass the reference ends on, 8-predictor argmin (DPP), winner's history, 4 x ds_write_b128", count(L[normal_blk[1]:tail_end + 1]))]
    print("# GC-ADPCM encoder: instruction budget of one wave-frame (round 9)\n")
    print("`gc_encode_persistent_kernel<8, false>`, static counts from hipcc's gfx950 listing of `vgaudio_amd/csrc/gc_encode_kernel.hip`")
    print("(`tools/isa_budget_gc.py`).  One wave-frame = 64 lanes = 8 channels x 8 predictors = 112 input samples.\n")
    print("| block of the hot frame | total | VALU | SALU | LDS | wait / nop |")
    print("|---|---:|---:|---:|---:|---:|")
    for name, c in rows:
        print("| %s | %d | %d | %d | %d | %d |" % (name, c["total"], c["VALU"], c["SALU"], c["LDS"], c["wait/nop"]))
    hot_valu = rows[0][1]["VALU"] + SHORT_SHARE * rows[1][1]["VALU"] + (1 - SHORT_SHARE) * rows[2][1]["VALU"] + rows[3][1]["VALU"]
    # the cold block: the third pass (short form) is the next cluster of 14 squares behind the hot tail that is a single pass
    third = [c for c in cluster(cv) if len(c) == 14]
    third_pass = count(L[prev_label(third[1][0]):next_label(third[1][-1])]) if len(third) > 1 else count([])
    print("\nCold block (third and later trips; %.3f of the wave-frames on the synthetic set): the third pass alone is %d VALU "
          "instructions for ~1.25 lanes of work; with its entry, loop and the frame's tail repeated behind it a plain visit executes "
          "~290 instructions more than a hot frame (the path was 385 until round 6: the bump loops of the generic resume point and the "
          "literal pass's hoisted set-up ran on every visit -- removing them changed nothing measurable: 146.1 against 145.9 ms).\n"
          % (COLD_RATE, third_pass["VALU"]))
    per_frame = hot_valu + COLD_RATE * (third_pass["VALU"] + 45)
    print("| per wave-frame (VALU) | instructions | lane-ops per input sample |")
    print("|---|---:|---:|")
    for name, v in (("the two passes (70 % short / 30 % with conversions)", SHORT_SHARE * rows[1][1]["VALU"] + (1 - SHORT_SHARE) * rows[2][1]["VALU"]),
                    ("row unpack, pre-scan, first scale", rows[0][1]["VALU"]),
                    ("select / argmin / commit", rows[3][1]["VALU"]),
                    ("cold block, %.3f x (third pass + ~45)" % COLD_RATE, COLD_RATE * (third_pass["VALU"] + 45)),
                    ("encoder wave, sum", per_frame)):
        print("| %s | %.0f | %.0f |" % (name, v, v * 64 / 112))
    print(TEXT)


TEXT = """
## What the budget says (round 9)

* Round 8's table is `profiles/r08_gc_encode_isa_budget.md`.  Its first row (87 VALU) took the frame to begin at the TILE's
  first label: the tool walked back a fixed number of lines and so counted the tile head (lane addresses, the first row's
  reads), which runs once per four frames.  The tool now takes the frame to begin at the label whose block opens with the next
  frame's six row reads; with that rule the parent of this round has 53 VALU in the row block and 519 per wave-frame.
* Row block 53 -> 41: the two history-dependent distances in the numerator domain (gc_encode_core.hpp N1: `v_sub` for the
  sign of D, `v_lshrrev`, `v_mad_i32_i24`, `v_ashrrev` on `in * 2048 + 1024 - P`, no unpacking of `in`, no quotient), both dot
  products in the clamped three-operand form (no `v_mov` of the zero), and the first scale from ONE bit length (F1-F4: two
  `v_med3`, `v_add`, `v_mul_i32_i24`, compare, `v_cndmask` with the shift folded in as SDWA, `v_or`, `v_ffbh`, `v_sub`; the
  +M / -M tie is one compare and a scalar branch).
* Passes 332 -> 328 / 365 -> 361: step 0 of both passes takes P0 and `in * 2048 + 1024 - P0` from the head.
* The helper wave's pre-scan is as it was (the numerator-domain form was measured and taken out: LABNOTES 14).
"""


def cluster(idx):
    out, cur = [], [idx[0]]
    for i in idx[1:]:
        if i - cur[-1] < 60:
            cur.append(i)
        else:
            out.append(cur)
            cur = [i]
    out.append(cur)
    return out


if __name__ == "__main__":
    main()
