#!/usr/bin/env python3
"""Per-frame instruction budget of gc_encode_persistent_kernel<8, false> from hipcc's ISA listing: where do
the ~409 lane-operations per input sample go against the ~240 the two passes x 8 predictors need?

The frame loop's basic blocks are found from the listing itself: a pair of quantise passes is the one block of the frame that
holds two passes' `v_cvt_pk_i16_i32` (clamp and history shift, one per sample step), with or without `v_cvt_f32_i32`; the
blocks between the loop's labels are classified by what they hold.
Prints static instruction counts per block of the HOT path of one frame (lane = (channel, predictor), CPW = 8: one wave-frame
= 8 channel-frames = 112 samples), the cold block's path for a plain third trip, the helper wave's loop per tile, and the
resulting lane-operations per sample with the measured rates (cold-block rate, short-pass share) filled in.

    python tools/isa_budget_gc.py > profiles/rNN_gc_encode_isa_budget.md

(Tables up to profiles/r08_gc_encode_isa_budget.md were made with an earlier frame-start rule that counted the tile head into
the frame's first row -- 87 VALU where this version says 53 for the same source; they cannot be reproduced with this version.)
"""
import collections
import os
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
    cv = [i for i, l in enumerate(L) if l.startswith("v_cvt_pk_i16_i32")]
    labels = [i for i, l in enumerate(L) if l.endswith(":")]
    prev_label = lambda i: max(j for j in labels if j <= i)
    next_label = lambda i: min(j for j in labels if j > i)
    # the frame's passes are the first code with an add with carry (round 10; the seam code inside the kernel keeps the old
    # pass).  The frame's first label: the nearest one in front of them whose block opens with the row reads of the NEXT
    # frame (six ds_read_b128); the frame's copy ends where the next block of that kind begins (the loop body holds two).
    first = next(i for i, l in enumerate(L) if l.startswith("v_addc_co_u32"))
    opens_frame = lambda j: sum(l.startswith("ds_read_b128") for l in L[j:j + 20]) >= 6
    frame_start = max(j for j in labels if j < first and opens_frame(j))
    frame_end = min(j for j in labels if j > first and opens_frame(j))
    # A pair of passes is the one basic block of the frame with two passes' clamp-and-shift instructions (v_cvt_pk_i16_i32: 28,
    # or a few less where the overflow-only pass drops its last; the cold block's passes come one to a block, 14): the pair with the f32 detour holds v_cvt_f32_i32, the short pair does not.  Found by
    # what the blocks hold, not by where they stand: since round 11 hipcc puts the short pair out of line behind the cold block.
    pairs = [(a, next_label(a)) for a in labels if frame_start <= a < frame_end
             and sum(l.startswith("v_cvt_pk_i16_i32") for l in L[a:next_label(a)]) >= 20]
    assert len(pairs) >= 2, "the listing does not look like the encoder's"
    has_cvt = lambda blk: any(l.startswith("v_cvt_f32_i32") for l in L[blk[0]:blk[1]])
    normal_blk = next(blk for blk in pairs if has_cvt(blk))
    short_blk = next(blk for blk in pairs if not has_cvt(blk))
    # the short pair's row runs on through the test of what the pair vouches for, to where it rejoins: the other pair's label
    # or the block's own s_branch
    end = short_blk[1]
    while end != normal_blk[0] and not L[end - 1].startswith("s_branch"):
        end = next_label(end)
    short_blk = (short_blk[0], end)
    # the tail ends with the jump to the next frame: an s_branch, or the conditional branch to the next frame's first label
    tail_end = normal_blk[1]
    while not (L[tail_end].startswith("s_branch") or (L[tail_end].startswith("s_cbranch") and L[tail_end].split()[1] + ":" == L[frame_end])):
        tail_end += 1
    # (what an execz branch jumps over -- the rare +M / -M tie's sequential pre-scan -- is not on the hot path)
    pre, skip_to = [], None
    for t in L[frame_start:min(short_blk[0], normal_blk[0])]:
        if skip_to:
            if t == skip_to + ":":
                skip_to = None
            continue
        pre.append(t)
        if t.startswith("s_cbranch_execz"):
            skip_to = t.split()[1]
    rows = [("row reads (6 x ds_read_b128) + pre-scan of the two history-dependent distances + first scale", count(pre)),
            ("the frame's two passes without the f32 detour, 28 sample steps, and the test of what they vouch for", count(L[short_blk[0]:short_blk[1]])),
            ("the same with the conversions (30 % of the wave-frames take these instead)", count(L[normal_blk[0]:normal_blk[1]])),
            ("the flags, the error block, 8-predictor argmin (DPP), winner's history, 4 x ds_write_b128", count(L[normal_blk[1]:tail_end + 1]))]
    print("# GC-ADPCM encoder: instruction budget of one wave-frame (round 11)\n")
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
## What the budget says (round 11)

* The parent's table, made with this version of the tool, is round 10's (`profiles/r10_gc_encode_isa_budget.md`): row block 50,
  passes 277 / 307, tail 62, cold block 77, encoder wave 475 VALU per wave-frame; tail 34 SALU.
* Tail 62 -> 40: the 21 selects between two result sets (14 nibbles, 7 history pairs) and the select of the overflow are gone --
  the final pass's registers ARE the frame's result (gc_encode_core.hpp T1, T2).  SALU 34 -> 38: the flags as before.
* Row block 50 -> 34: one pass's constants (shift, bias, -Z, two clamp bounds) are formed in front of the pair instead of two.
* Passes 277 -> 276 / 307 -> 321: the second pass builds its constants from sp2 behind the first (select of the scale, shift for
  -Z, two adds, the bias), the overflow-only pass drops its last clamp-and-shift and every register copy of its nibbles.
* Encoder wave 475 -> 440: **-35 VALU per wave-frame** (-39 on a short frame, -24 on one with the conversions).  As in round 10
  the tool counts the block in front of the conversions pair into the row block although the short path jumps over it
  (parent: 20 VALU there, now 4), so a short frame saves about 8 fewer than the table says.
* hipcc now places the short pair out of line (behind the cold block, a branch there and one back); the tool finds the pairs
  by what their blocks hold.
* Step 2 of the round (the flags as compares and lane-mask logic, one bit for the branch; measured, not kept -- LABNOTES 16.3):
  tail 40 -> 36 VALU and 38 -> 12 SALU, both exec-mask diamonds gone.
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
