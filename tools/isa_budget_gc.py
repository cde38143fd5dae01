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
    # first frame of the loop body (row set A): short pair of passes (2 x 14 sample steps), then the normal pair.  The passes'
    # extent is taken from the fourteen v_cvt_pk_i16_i32 of each -- clamp and history shift, on the chain.
    if any(l.startswith("v_addc_co_u32") for l in L):
        # round 10: the frame's passes are the first code with an add with carry (the seam code inside the kernel keeps the
        # old pass); the hot passes form no squares any more -- one error block of seven stands in the frame's tail
        first = next(i for i, l in enumerate(L) if l.startswith("v_addc_co_u32"))
        cv = [i for i, l in enumerate(L) if l.startswith("v_cvt_pk_i16_i32") and i > first - 40]
        assert len(cv) >= 56, "the listing does not look like the encoder's"
        inside = lambda a, b: [i for i in sq if a <= i <= b + 60]
        short_a, short_b = cv[0], max([cv[27]] + (inside(cv[0], cv[27]) if len(inside(cv[0], cv[55])) >= 28 else []))
        normal_a, normal_b = cv[28], max([cv[55]] + (inside(cv[28], cv[55]) if len(inside(cv[0], cv[55])) >= 28 else []))
    else:
        assert len(sq) >= 28, "the listing does not look like the encoder's"
        # (hipcc sinks the short pair's squares behind the passes, into a block of their own: stretched over the squares)
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
    print("# GC-ADPCM encoder: instruction budget of one wave-frame (round 10)\n")
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
## What the budget says (round 10)

* Round 9's table is `profiles/r09_gc_encode_isa_budget.md` (same tool, parent of this round): row block 41, passes 328 / 361,
  tail 43, cold block 81, encoder wave 503 VALU per wave-frame.
* Passes 328 -> 277 / 361 -> 307.  Step 1 (gc_encode_core.hpp B1-B5): the sample step is `v_dot2`, `v_sub_co`, `v_addc_co`,
  shift, `v_med3`, `P >> 11`, `v_lshl_add`, `v_cvt_pk` -- 8 where it was 9 (`v_sub`, `v_lshrrev`, `v_add3`), -23 / -26 per pair
  of passes (step 0 keeps a `v_cndmask` of the borrow the two passes share).  hipcc puts `s_nop 1` between the carry pair
  (a VALU write of an SGPR read by the next VALU): 66 / 51 wait / nop lines against 27 / 28.  Step 2: the passes form no
  squares (-28: 2 x 7 `v_pk_sub_i16` + `v_dot2`).
* Tail 43 -> 62: seven selects of the history pairs (the seventh is the winner's history: one select it had already) and one
  error block of 7 + 7.  Steps 1 + 2 together: -51 in the passes, +19 in the tail.
* Row block 41 -> 50: per pass one shift for -Z and two adds for the clamp bounds (6), the borrow of the shared step 0.  The
  tool counts the block in front of the conversions pair (10 VALU: its copy of the pass constants) into this row although
  the short path jumps over it, so a frame of the short kind executes about 5 fewer than the table says.
* Cold block 81 -> 77: the third pass 190 -> 178.
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
