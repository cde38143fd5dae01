#!/usr/bin/env python3
"""Per-frame instruction budget of gc_encode_persistent_kernel<8, false> from hipcc's ISA listing: where do
the ~409 lane-operations per input sample go against the ~240 the two passes x 8 predictors need?

The frame loop's basic blocks are found from the listing itself: a pair of quantise passes is the one block of the frame that
holds two passes' `v_cvt_pk_i16_i32` (clamp and history shift, one per sample step), with or without `v_cvt_f32_i32`; the
blocks between the loop's labels are classified by what they hold.
Prints static instruction counts per block of the HOT path of one frame (lane = (channel, predictor), CPW = 8: one wave-frame
= 8 channel-frames = 112 samples), the cold block's path for a plain third trip, the helper wave's loop per tile, and the
resulting lane-operations per sample with the measured rates (cold-block rate, short-pass share) filled in.

    python tools/isa_budget_gc.py [--src other/gc_encode_kernel.hip] [--shape self] [-DNAME=VALUE ...] > profiles/rNN_gc_encode_isa_budget.md

--shape self (round 13): the same table for gc_encode_self_served_kernel<false> -- the one-wave workgroups that are helper and
encoder of their eight channel slots -- and, in place of the helper wave's loop, the static counts of that kernel's tile
boundary: the blocks of the tile loop outside the frame loop (next tile's loads, flush, the compute half of prepare).

Since round 12 the listing is made with the product's own options for the file (vgaudio_amd/build.py FILE_FLAGS; until then
with the common ones only), and the tool also counts the scratch instructions (spill stores and reloads) per block of the
frame, for the uniform and the ragged instantiation: the blocks of the frame loop are the ones hipcc's loop comments put under
the first depth-3 loop header of the kernel, wherever they stand in the listing.  --src: the same for another copy of the
kernel file (a parent's, say), compiled against this tree's headers.

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
    sys.path.insert(0, ROOT)
    from vgaudio_amd.build import FILE_FLAGS                  # the product's per-file code generation options
    src = os.path.abspath(sys.argv[sys.argv.index("--src") + 1]) if "--src" in sys.argv else SRC
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + FILE_FLAGS.get("gc_encode_kernel.hip", []) + ["-I", os.path.dirname(SRC)] +
                       [a for a in sys.argv[1:] if a.startswith("-D")] +
                       ["--save-temps=obj", "-c", src, "-o", os.path.join(tmp, "k.o")], check=True, cwd=tmp,
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


def scratch_by_block(raw, name):
    """Scratch instructions of one kernel by where they stand: {region: count}, and the in-loop ones one by one.  The frame loop
    is the kernel's first depth-3 loop (piece queue > tiles > frames); hipcc's comments name every block's innermost loop."""
    import re
    a = next(i for i, l in enumerate(raw) if l.startswith("_Z") and name in l and l.split(";")[0].rstrip().endswith(":"))
    b = next(i for i in range(a, len(raw)) if "s_endpgm" in raw[i])
    frame_hdr, tile_hdr, nested, tile_nested, where, lab = None, None, set(), set(), "prologue, seams, epilogue", None
    regions, inside = collections.OrderedDict(), []
    tile_code = []                                                   # every instruction of the tile loop outside the frame loop
    for key in ("frame loop: the frame's pairs of passes", "frame loop: the cold block's passes", "frame loop: row reads, first scale, flags, tail, the cold block's other code",
                "tile head (once per tile, outside the frame loop)", "prologue, seams, epilogue"):
        regions[key] = 0
    i = a + 1
    while i < b:
        m = re.match(r"^(\.LBB\d+_\d+):", raw[i])
        if m:
            lab = m.group(1)[2:]
            j, com = i + 1, raw[i]
            while j < b and raw[j].lstrip().startswith(";"):
                com += raw[j]
                j += 1
            if frame_hdr is None and "This Loop Header: Depth=2" in com:
                tile_hdr = lab                                       # (the last depth-2 header in front of the frame loop)
                tile_nested = {lab}
            if frame_hdr is None and "This Loop Header: Depth=3" in com:
                frame_hdr = lab
            if frame_hdr and (lab == frame_hdr or re.search(r"Parent Loop %s\b" % frame_hdr, com)):
                nested.add(lab)
            inner = re.search(r"in Loop: Header=(BB\d+_\d+)", com)
            in_frame = lab in nested or (inner is not None and inner.group(1) in nested)
            in_tile = not in_frame and (lab in tile_nested or (inner is not None and inner.group(1) in tile_nested))
            end = next((k for k in range(j, b) if re.match(r"^\.LBB\d+_\d+:", raw[k])), b)
            cvt = sum(l.lstrip().startswith("v_cvt_pk_i16_i32") for l in raw[j:end])
            if in_frame:
                where = ("frame loop: the frame's pairs of passes" if cvt >= 20 else "frame loop: the cold block's passes" if cvt >= 13
                         else "frame loop: row reads, first scale, flags, tail, the cold block's other code")
            elif in_tile:
                where = "tile head (once per tile, outside the frame loop)"
            else:
                where = "prologue, seams, epilogue"
        elif raw[i].lstrip().startswith("scratch_"):
            regions[where] += 1
            if where.startswith("frame loop"):
                inside.append("%s: %s" % (lab, raw[i].split(";")[0].strip()))
        if where.startswith("tile head") and not m:
            t = raw[i].split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                tile_code.append(t)
        i += 1
    scratch_by_block.tile_code = tile_code
    return regions, inside, frame_hdr


def resources(raw, name):
    """VGPRs, spill slots and scratch bytes per lane from the kernel's .amdhsa / metadata comment block."""
    import re
    a = next(i for i, l in enumerate(raw) if l.startswith("_Z") and name in l and l.split(";")[0].rstrip().endswith(":"))
    out = {}
    for l in raw[a:]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                break
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
    RAW = listing()
    self_shape = "--shape" in sys.argv and sys.argv[sys.argv.index("--shape") + 1] == "self"
    uniform, ragged = (("gc_encode_self_served_kernelILb0E", "gc_encode_self_served_kernelILb1E") if self_shape
                       else ("gc_encode_persistent_kernelILi8ELb0E", "gc_encode_persistent_kernelILi8ELb1E"))
    nice_name = "gc_encode_self_served_kernel<%s>" if self_shape else "gc_encode_persistent_kernel<8, %s>"
    L = kernel(RAW, uniform)
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
    print("# GC-ADPCM encoder: instruction budget of one wave-frame (round 13)\n")
    print("`" + nice_name % "false" + "`, static counts from hipcc's gfx950 listing of `vgaudio_amd/csrc/gc_encode_kernel.hip`")
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
    # scratch (spill stores and reloads) by where it stands, uniform and ragged instantiation
    print("\n## Registers and scratch instructions by block\n")
    for nice, mangled in ((nice_name % "false", uniform), (nice_name % "true", ragged)):
        regions, inside, hdr = scratch_by_block(RAW, mangled)
        if self_shape:
            c = count(scratch_by_block.tile_code)
            print("`%s`, tile boundary (the blocks of the tile loop outside the frame loop, every branch counted once -- the partial last "
                  "frame's byte loops among them): %d instructions, %d VALU, %d SALU, %d LDS, %d VMEM per tile of 8 frames x 8 channel slots.\n"
                  % (nice, c["total"], c["VALU"], c["SALU"], c["LDS"], c["VMEM"]))
        res = resources(RAW, mangled)
        print("`%s`: %d VGPRs, %d waves per SIMD, %d B of scratch per lane, %d B of LDS per workgroup; frame loop header `.L%s`.\n"
              % (nice, res.get("NumVgprs", -1), res.get("Occupancy", -1), res.get("ScratchSize", -1), res.get("LDSByteSize", -1), hdr))
        print("| where | scratch instructions |")
        print("|---|---:|")
        for k, v in regions.items():
            print("| %s | %d |" % (k, v))
        print("| **frame loop, header to back edge, cold block included** | **%d** |\n" % len(inside))
        for t in inside:
            print("* in the frame loop: `%s`" % t)
    if "--src" not in sys.argv and not any(a.startswith("-D") for a in sys.argv[1:]):
        print(TEXT_SELF if self_shape else TEXT)


TEXT_SELF = """
## What the budget says (round 13, written before the GPU run)

* The frame loop is the 2 + 1 shape's, instruction for instruction: row block 33, passes 276 / 321, tail 37 VALU, encoder role
  436 VALU per wave-frame (`gc_encode_persistent_kernel<8, false>` from the same source reads the same, 166 VGPRs).
* The tile boundary stands where the helper wave's loop stood.  A tile is 8 frames x 8 channel slots = 8 wave-frames; the helper's
  tile of 4 frames x 16 slots is 8 wave-frames as well: 762 VALU there (95 per wave-frame), at most 871 here (109 per wave-frame;
  the static count holds the partial last frame's byte loops and both sides of every branch, a full tile executes fewer).  What
  is new in it: eight `ds_bpermute` for the coefficient pairs of the helper role, the lane's slot address once more, and the
  clamped frame index formed twice (load and compute).
* 167 VGPRs with the next tile's seven dwords held across the frame loop, no scratch anywhere in the kernel, 12 612 B of LDS
  per workgroup: twelve workgroups are 151 344 B of the compute unit's 163 840 (13 312 B each if the allocation is in steps
  of 512 B: 159 744).
* Prediction, written down before the GPU run.  Instructions per launch: encoder role unchanged, helper role 95 -> 100-109 per
  wave-frame, so SQ_INSTS_VALU +1 to +2.6 % (531 -> 536-545 per wave-frame).  Time goes as instructions / busy fraction: if three
  like waves per SIMD lift SQ_ACTIVE_INST_VALU / issue slots from 0.90 to 0.97 the launch is 112 ms x 1.026 x 0.90 / 0.97 = 106.6 ms
  at the worst instruction count (-5 ms) and 105 ms at the best; if the busy fraction does not move, the launch is 1-3 ms SLOWER
  and the shape stays behind the test hook.  Measured: LABNOTES 18.
"""

TEXT = """
## What the budget says (round 12)

* The parent's table (`profiles/r11_gc_encode_isa_budget.md`, made with the common options only): row block 34, passes 276 / 321,
  tail 40 VALU and 38 SALU, cold block 77, encoder wave 440 VALU per wave-frame.  With the product's per-file options, which
  this version of the tool uses, the parent's rows and passes read the same; the rule that finds the end of the tail runs
  past the parent's flag diamonds there (`--src` on the parent's file), so the parent's tail is quoted from round 11.
* The flags as one bit (`frame_goes_cold`): the tail's two exec-mask diamonds are gone, the single flags are formed inside the
  cold branch: tail 40 -> 37 VALU, 38 -> 12 SALU.
* One LDS slot per (channel slot, frame) -- row, pre-scan words, record -- reached from ONE address register with immediate
  offsets: the row block forms one address where it formed three (34 -> 33 VALU with the `v_mov` that keeps the pre-scan
  word's index opaque per frame); the tile head derives the address from the hardware's lane number.
* Prediction, written down before the GPU run: encoder wave 440 -> 436 VALU per wave-frame (437 in the four-waves build), SALU -26 in the tail; at three
  waves per SIMD that is worth what round 11's step 2 measured (about 1 ms) plus whatever the row reads gain from landing in
  disjoint banks.  Measured: LABNOTES 17.
* The build at four waves per SIMD (`-DVGA_GC_PERSISTENT_WAVES_PER_EU=4,4`; table below the kept build's when given): 128 VGPRs,
  no scratch instruction between the frame loop's header and its back edge in either instantiation, none in the tile head;
  what is left stands in the piece prologue and the seam code.  Measured and not kept.
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
