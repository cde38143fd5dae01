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
Round 14: that boundary split by block -- load and unpack, row, pre-scan, flush and pack, bookkeeping -- by the source line of
every instruction (the listing is made with -gline-tables-only; tile_blocks), the frame loop's instruction count with a digest
of its mnemonics (to hold a change against its parent's, --src), and the kernel's instruction count.

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
        # (line tables only: the .loc directives the tile boundary's split by block reads; they change no instruction)
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-gline-tables-only"] + FILE_FLAGS.get("gc_encode_kernel.hip", []) + ["-I", os.path.dirname(SRC)] +
                       [a for a in sys.argv[1:] if a.startswith("-D")] +
                       ["--save-temps=obj", "-c", src, "-o", os.path.join(tmp, "k.o")], check=True, cwd=tmp,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f][0]
        listing.src = src
        return open(os.path.join(tmp, s)).read().split("\n")


def kernel(lines, name):
    a = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l and l.split(";")[0].rstrip().endswith(":"))
    b = next(i for i in range(a, len(lines)) if "s_endpgm" in lines[i])
    out = []
    for l in lines[a + 1:b + 1]:
        t = l.split(";")[0].rstrip()
        if not t.strip() or t.strip().startswith((".p2align", ".", "//")) and not t.strip().endswith(":"):
            continue
        if t.strip().endswith(":") and not t.strip().startswith(".LBB"):   # (.Ltmp labels of the line tables are no block boundaries)
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
    tile_loc, cur_loc, frame_ops = [], (0, 0), []                    # ... its (file number, line) by the .loc in force; the frame loop's mnemonics
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
        loc = re.match(r"^\s*\.loc\s+(\d+)\s+(\d+)", raw[i])
        if loc:
            cur_loc = (int(loc.group(1)), int(loc.group(2)))
        if not m:
            t = raw[i].split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                if where.startswith("tile head"):
                    tile_code.append(t)
                    tile_loc.append(cur_loc)
                elif where.startswith("frame loop"):
                    frame_ops.append(t.split()[0])
        i += 1
    scratch_by_block.tile_code = tile_code
    scratch_by_block.tile_loc = tile_loc
    scratch_by_block.frame_ops = frame_ops
    return regions, inside, frame_hdr


TILE_BLOCKS = ("load and unpack", "row", "pre-scan", "flush and pack", "bookkeeping")


def tile_blocks(raw, tile_code, tile_loc):
    """The tile boundary's instructions by the source line their .loc names (round 14): the helper role's lambdas of the kernel
    file and the functions of gc_encode_core.hpp they call.  load and unpack: load_frame and prepare_self's unpack; row: the
    pairs and the pass's row into the LDS slot (prepare_from up to the pre-scan's pairs); pre-scan: the rest of prepare_from
    with the header's dot products, quotients, max / min and packing; flush and pack: flush and pack_frame_mod16; bookkeeping:
    everything else (the loop, the fences and waits, the coefficient pairs' ds_bpermute, the item's end)."""
    import re
    files = {}
    for l in raw:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    src = open(listing.src).read().split("\n")

    def extent(opening, closing="    };"):
        a = next(i for i, l in enumerate(src) if opening in l)
        pad = len(src[a]) - len(src[a].lstrip())
        b = next(i for i in range(a + 1, len(src)) if src[i].rstrip() == " " * pad + "};")
        return a + 1, b + 1                                          # 1-based, inclusive
    load, prep, flush, pself = (extent("auto load_frame = "), extent("auto prepare_from = "), extent("auto flush = "),
                                extent("auto prepare_self = "))
    pairs = next(i for i in range(prep[0], prep[1]) if "uint32_t pair[12];" in src[i]) + 1
    core = open(os.path.join(os.path.dirname(SRC), "gc_encode_core.hpp")).read().split("\n")

    def core_fn(line):                                               # the function of the header a line stands in
        for i in range(min(line, len(core)) - 1, -1, -1):
            m = re.match(r"^VGA_HD\s+[\w:<> ]+?\b(\w+)\(", core[i])
            if m:
                return m.group(1)
        return ""
    out = {k: [] for k in TILE_BLOCKS}
    for t, (fno, line) in zip(tile_code, tile_loc):
        name = files.get(fno, "")
        if name == os.path.basename(listing.src):
            where = ("load and unpack" if load[0] <= line <= load[1] else
                     "row" if prep[0] <= line < pairs else "pre-scan" if pairs <= line <= prep[1] else
                     "flush and pack" if flush[0] <= line <= flush[1] else
                     "load and unpack" if pself[0] <= line <= pself[1] and "__shfl" not in src[line - 1] and "prepare_from" not in src[line - 1]
                     else "bookkeeping")
        elif name == "gc_encode_core.hpp":
            fn = core_fn(line)
            where = ("pre-scan" if fn in ("prescan_numer_word", "numer_adjust", "dot2_i16", "dot2_i16_wrap", "div2048", "sat_pack16", "imax", "imin",
                                          "clamp16i", "pk_sub_sat_i16", "med3_i32") else
                     "row" if fn == "pass_b_row" else "flush and pack" if fn.startswith("pack_frame") else "bookkeeping")
        else:
            where = "bookkeeping"
        out[where].append(t)
    return out


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
    print("# GC-ADPCM encoder: instruction budget of one wave-frame (round 14)\n")
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
            print("| block of the tile boundary | total | VALU | SALU | LDS | VMEM | wait / nop |")
            print("|---|---:|---:|---:|---:|---:|---:|")
            for k, blk in tile_blocks(RAW, scratch_by_block.tile_code, scratch_by_block.tile_loc).items():
                b = count(blk)
                print("| %s | %d | %d | %d | %d | %d | %d |" % (k, b["total"], b["VALU"], b["SALU"], b["LDS"], b["VMEM"], b["wait/nop"]))
            import hashlib
            ops = scratch_by_block.frame_ops
            print("\nFrame loop, header to back edge: %d instructions; SHA-1 of their mnemonics sorted `%s`, in listing order `%s`; the "
                  "whole kernel: %d instructions.\n"
                  % (len(ops), hashlib.sha1(" ".join(sorted(ops)).encode()).hexdigest()[:16], hashlib.sha1(" ".join(ops).encode()).hexdigest()[:16],
                     sum(not l.endswith(":") for l in kernel(RAW, mangled))))
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
## What the budget says (round 14, written before the GPU runs it speaks of)

* The tile boundary by block (the table above; the split follows the `.loc` line of every instruction, so an instruction the
  scheduler moved or merged counts where its line says).  Static VALU per tile of 8 wave-frames, both sides of every branch and
  the partial last frame's byte loops counted: parent 871 (`--src` on the parent's file: pre-scan 703), the numerator form as
  the issue words it -- dot product, subtract, sign bit, `v_mad_u32_u24`, `v_max3` / `v_min3` over pairs, 5 per term -- 682, the
  form as committed -- dot product, add, `v_med3_i32` (gc_encode_core.hpp N7), 4 per term, one `v_cvt_pk_i16_i32` for both clamps
  and the packing -- **586**: pre-scan 703 -> 418, the rolled fallback loop of a wave with a hostile channel among them, which a clean
  wave never executes; the other blocks sum to 168 on both sides.  The whole kernel: 13 187 -> 12 584 instructions (the two forms side by side do
  not grow it: the fallback is a loop rolled over the predictors).
* What the issue's item 3 names does not survive in this listing: the row is formed from the loaded pairs ((w << 16) >> 5, and
  an SDWA shift of the high half), there is no second unpack; the slot address is one `v_mad_u32_u24` shared by `flush` and
  `prepare_from`; the clamped frame index is formed once per load (`v_lshl_or`, `v_min`), `flush` has the unclamped index of its
  own tile.  Nothing was changed in the source for them.
* Conditions: 167 VGPRs (168 in the ragged instantiation), three waves per SIMD, no scratch instruction anywhere in the kernel.
  The frame loop holds the parent's 6406 instructions -- the same mnemonics with the same counts (the SHA-1 of the sorted list
  is the parent's); hipcc schedules a few of them (`v_or_b32` / `v_lshlrev_b32` of the record's packing, the `s_nop` in front of a
  dot product's reader) in another order, so the digest in listing order differs.
* Prediction.  Static: 871 -> 586 VALU per tile, -285, that is -35.6 per wave-frame of about 561 (SQ_INSTS_VALU 59.07 G per
  launch, round 13): **SQ_INSTS_VALU -6.3 %, to about 55.3 G**; executed instructions fall a little further (a clean wave runs
  neither form's fallback).  At the parent's busy fraction (0.988) the 105.3 ms kernel would take about **98.6 ms (-6.7 ms)**.
  (The form is compiled into the self-served shape only: every kernel with a helper wave compiles to the parent's
  instruction count, `profiles/r14_kernel_resources_gc_encode.txt`.)
  Session 1 of `profiles/r14_encode_ab.log` measured the issue's five-per-term form (-189 static) at -1.84 ms of the encode
  call where the same reckoning gave -4.5: at that exchange rate the form as committed is worth about **-2.8 ms**.  Measured:
  LABNOTES 19.
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
