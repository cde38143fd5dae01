"""Independent restatement of the reference's HPS, IDSP and GENH containers (VGAudio/Containers/Hps/HpsWriter.cs,
HpsReader.cs, Idsp/IdspWriter.cs, IdspReader.cs, Genh/GenhReader.cs) in plain Python + struct, for the tests: layouts,
block maps, byte images and parses.  Nothing here calls the library.  The reference has no GENH writer; genh_image
builds test files in the layout GenhReader reads."""
import struct


# GcAdpcmMath.cs:11-47, Helpers.cs:71-83
def nibble_count_to_sample_count(n):
    return 14 * (n // 16) + (0 if n % 16 < 2 else n % 16 - 2)


def sample_count_to_nibble_count(s):
    return 16 * (s // 14) + (0 if s % 14 == 0 else s % 14 + 2)


def nibble_to_sample(n):
    return 14 * (n // 16) + n % 16 - 2


def sample_to_nibble(s):
    return 16 * (s // 14) + s % 14 + 2


def bytes_of(s):
    n = sample_count_to_nibble_count(s)
    return n // 2 + n % 2


def byte_count_to_sample_count(b):
    return nibble_count_to_sample_count(b * 2)


def next_multiple(v, m):
    return v if m <= 0 or v % m == 0 else v + m - v % m


def div_round_up(v, d):
    return -(-v // d)


def aligned_loop(looping, ls, le, sample_count, multiple):
    """GcAdpcmFormat.cs:14-18 / GcAdpcmAlignment: (loop start, loop end, format sample count, channel sample count)"""
    if not looping:
        return 0, 0, sample_count, sample_count
    if multiple and ls % multiple:
        shift = next_multiple(ls, multiple) - ls
        return ls + shift, le + shift, le + shift, le + shift
    return ls, le, sample_count, sample_count


# ---------------------------------------------------------------- HPS
class CannotWrite(Exception):
    """the reference's writer throws"""


def hps_layout(nch, sample_count, looping=False, loop_start=0, loop_end=0):
    """HpsWriter.SetupWriter + CreateBlockMap"""
    header = next_multiple(max(0x80, 0x10 + 0x38 * nch), 0x20)
    channel_size = next_multiple(0x10000 // nch, 0x20)
    alignment = byte_count_to_sample_count(channel_size)
    ls, le, sc, _ = aligned_loop(looping, loop_start, loop_end, sample_count, alignment)
    nibbles = sample_count_to_nibble_count(sc)
    mcb = channel_size * nch // nch * 2
    count = div_round_up(nibbles, mcb)
    loop_block = sample_to_nibble(ls) // mcb if looping else count - 1
    sizes, nib = [], 0
    while len(sizes) < loop_block:
        sizes.append((nib, mcb))
        nib += mcb
    while nib < nibbles:
        left = nibbles - nib
        size = min(left, next_multiple(div_round_up(left, count - len(sizes)), 0x40))
        sizes.append((nib, size))
        nib += size
    blocks, off = [], header
    for nib, size in sizes:
        cs = div_round_up(size, 2)
        written = next_multiple(cs, 0x20) * nch
        total = next_multiple(4 + 8 * nch, 0x20) + written
        blocks.append(dict(offset=off, start_sample=nibble_to_sample(nib + 2), byte_in_index=nib // 2, channel_size=cs,
                           written_size=written, total_size=total, end_nibble=size - 1))
        off += total
    for a, b in zip(blocks, blocks[1:]):
        a["next_offset"] = b["offset"]
    if blocks:
        blocks[-1]["next_offset"] = blocks[loop_block]["offset"] if looping else -1
    return dict(header_size=header, channel_size=channel_size, alignment=alignment, loop_start=ls, loop_end=le,
                sample_count=sc, loop_block=loop_block, blocks=blocks, file_size=off)


def hps_image(sample_rate, adpcm, coefs, gain, start, hist, looping=False, loop_start=0, loop_end=0, unaligned_count=None):
    """The bytes HpsWriter writes: adpcm[c] = GetAdpcmAudio() (aligned), start[c] = (ps, h1, h2), hist[c] = the Pcm field
    (None: zeros).  loop points are the format's unaligned ones; raises CannotWrite where the reference throws."""
    nch = len(adpcm)
    L = hps_layout(nch, unaligned_count, looping, loop_start, loop_end)
    if not L["blocks"]:
        raise CannotWrite("no block")
    out = bytearray(L["file_size"])
    pos = 0

    def put(fmt, *v):
        nonlocal pos
        b = struct.pack(">" + fmt, *v)
        if pos + len(b) > len(out):                       # MemoryStream over byte[FileSize] cannot grow
            raise CannotWrite("write past the end of the image")
        out[pos:pos + len(b)] = b
        pos += len(b)

    put("8s", b" HALPST\0")
    put("ii", sample_rate, nch)
    for c in range(nch):
        put("iiii", 0x10000, sample_to_nibble(0), sample_to_nibble(L["sample_count"] - 1), sample_to_nibble(0))
        put("16h", *coefs[c])
        put("h", gain[c])
        put("3h", *start[c])
    pos = L["header_size"]
    for B in L["blocks"]:
        put("iii", B["written_size"], B["end_nibble"], B["next_offset"])
        s = B["start_sample"]
        for c in range(nch):
            h = hist[c] if hist is not None else None

            def at(i):
                if i < 0 or h is None:
                    return 0
                if i >= len(h):
                    raise CannotWrite("IndexOutOfRangeException in GetHist")
                return int(h[i])
            put("hhhh", adpcm[c][s // 14 * 8], at(s - 1), at(s - 2), 0)
        pos = next_multiple(pos, 0x20)
        for c in range(nch):
            chunk = bytes(adpcm[c][B["byte_in_index"]:B["byte_in_index"] + B["channel_size"]])
            if len(chunk) != B["channel_size"]:
                raise CannotWrite("short audio")
            put("%ds" % len(chunk), chunk)
            pos = next_multiple(pos, 0x20)
    return bytes(out)


def hps_parse(data):
    """HpsReader.ReadFile + ToAudioStream: dict with the channels' audio concatenated"""
    rd = lambda f, at: struct.unpack_from(">" + f, data, at)
    if data[:8] != b" HALPST\0":
        raise ValueError("magic")
    rate, nch = rd("ii", 8)
    chans, pos = [], 16
    for c in range(nch):
        mbs, _, end, _ = rd("iiii", pos)
        coefs = list(rd("16h", pos + 16))
        gain, = rd("h", pos + 48)
        start = list(rd("3h", pos + 50))
        chans.append(dict(max_block_size=mbs, end_address=end, coefs=coefs, gain=gain, start=start))
        pos += 0x38
    nxt, cur, blocks = next_multiple(max(0x80, pos), 0x20), 0, []
    while nxt > cur:
        cur = nxt
        size, final, next_off = rd("iii", cur)
        ctx = [list(rd("3h", cur + 12 + 8 * c)) for c in range(nch)]
        audio_start = next_multiple(cur + 12 + 8 * nch, 0x20)
        n = (final + 1 + 1) // 2
        audio = [bytes(data[audio_start + size // nch * c: audio_start + size // nch * c + n]) for c in range(nch)]
        blocks.append(dict(offset=cur, size=size, final=final, next=next_off, ctx=ctx, audio=audio, audio_start=audio_start))
        nxt = next_off
    sc = nibble_to_sample(chans[0]["end_address"]) + 1
    if any(nibble_to_sample(c["end_address"]) + 1 != sc for c in chans):
        raise ValueError("Channels have differing sample counts")
    looping, loop_start, loop_ctx = False, 0, [[0, 0, 0]] * nch
    start_off, nib = blocks[-1]["next"], 0
    if start_off != -1:
        for b in blocks:
            if b["offset"] == start_off:
                looping, loop_start, loop_ctx = True, nibble_count_to_sample_count(nib), b["ctx"]
            nib += b["final"] + 1
    audio = [b"".join(b["audio"][c] for b in blocks) for c in range(nch)]
    return dict(sample_rate=rate, channel_count=nch, sample_count=sc, looping=looping, loop_start=loop_start,
                channels=chans, loop_context=loop_ctx, blocks=blocks, audio=audio)


# ---------------------------------------------------------------- IDSP
def interleave(rows, il, out_size):
    """Interleave.cs:43-78 over a zeroed buffer"""
    n = len(rows)
    in_size = len(rows[0])
    out = bytearray(out_size * n)
    in_b, out_b = div_round_up(in_size, il), div_round_up(out_size, il)
    last_in, last_out = in_size - (in_b - 1) * il, out_size - (out_b - 1) * il
    for b in range(min(in_b, out_b)):
        ci = last_in if b == in_b - 1 else il
        co = last_out if b == out_b - 1 else il
        k = min(ci, co)
        for i, r in enumerate(rows):
            at = il * b * n + co * i
            out[at:at + k] = r[il * b:il * b + k]
    return bytes(out)


def deinterleave(data, length, il, n, out_size=-1):
    """Interleave.cs:118-167 (the stream form) from data[0:length]"""
    in_size = length // n
    out_size = in_size if out_size == -1 else out_size
    outs = [bytearray(out_size) for _ in range(n)]
    in_b, out_b = div_round_up(in_size, il), div_round_up(out_size, il)
    last_in, last_out = in_size - (in_b - 1) * il, out_size - (out_b - 1) * il
    for b in range(min(in_b, out_b)):
        ci = last_in if b == in_b - 1 else il
        co = last_out if b == out_b - 1 else il
        k = min(ci, co)
        for o in range(n):
            at = il * b * n + ci * o
            outs[o][il * b:il * b + k] = data[at:at + k]
    return [bytes(o) for o in outs]


def idsp_layout(nch, sample_count, looping, loop_start, loop_end, block_size=0x10, trim=True):
    """IdspWriter.cs:17-51"""
    if block_size < 0 or block_size % 8:
        raise ValueError("block size")
    mult = byte_count_to_sample_count(block_size) if block_size else 0
    ls, le, fsc, csc = aligned_loop(looping, loop_start, loop_end, sample_count, mult)
    sc = le if trim and looping else max(fsc, le)
    ads = next_multiple(bytes_of(sc), 8 if block_size == 0 else block_size)
    il = ads if block_size == 0 else block_size
    header = 0x40 + 0x60 * nch
    return dict(loop_start=ls, loop_end=le, sample_count=sc, channel_sample_count=csc, audio_data_size=ads, interleave=il,
                header_size=header, file_size=header + ads * nch, start_addr=sample_to_nibble(ls if looping else 0),
                end_addr=sample_to_nibble(le if looping else sc - 1))


def idsp_image(sample_rate, adpcm, coefs, gain, start, loop, looping, loop_start, loop_end, unaligned_count,
               block_size=0x10, trim=True):
    """IdspWriter.WriteHeader + WriteData; adpcm[c] = GetAdpcmAudio() after the build"""
    nch = len(adpcm)
    L = idsp_layout(nch, unaligned_count, looping, loop_start, loop_end, block_size, trim)
    out = bytearray(L["file_size"])
    struct.pack_into(">4siiiiiiiiiii", out, 0, b"IDSP", 0, nch, sample_rate, L["sample_count"],
                     L["loop_start"], L["loop_end"], block_size, 0x40, 0x60, L["header_size"], L["audio_data_size"])
    for c in range(nch):
        struct.pack_into(">iiihhiii16hh3h3h", out, 0x40 + 0x60 * c, L["channel_sample_count"],
                         sample_count_to_nibble_count(L["channel_sample_count"]), sample_rate, 1 if looping else 0, 0,
                         L["start_addr"], L["end_addr"], sample_to_nibble(0), *coefs[c], gain[c], *start[c], *loop[c])
    body = interleave([bytes(a) for a in adpcm], L["interleave"], L["audio_data_size"])
    out[L["header_size"]:L["header_size"] + len(body)] = body
    return bytes(out)


def idsp_parse(data):
    """IdspReader.ReadFile"""
    if data[:4] != b"IDSP":
        raise ValueError("magic")
    nch, rate, sc, ls, le, il, hs, cis, ado, adl = struct.unpack_from(">10i", data, 8)
    chans = []
    for c in range(nch):
        at = hs + c * cis
        csc, nib, crate, lp, _, sa, ea, ca = struct.unpack_from(">iiihhiii", data, at)
        v = struct.unpack_from(">16hh3h3h", data, at + 28)
        chans.append(dict(sample_count=csc, looping=lp == 1, start_address=sa, end_address=ea, coefs=list(v[:16]), gain=v[16],
                          start=list(v[17:20]), loop=list(v[20:23])))
    interleave_ = adl if il == 0 else il
    audio = deinterleave(data[ado:], nch * adl, interleave_, nch, bytes_of(sc))
    return dict(channel_count=nch, sample_rate=rate, sample_count=sc, loop_start=ls, loop_end=le, interleave_size=il,
                header_size=hs, channel_info_size=cis, audio_data_offset=ado, audio_data_length=adl,
                looping=any(c["looping"] for c in chans), channels=chans, audio=audio)


# ---------------------------------------------------------------- GENH
def genh_image(sample_rate, adpcm, coefs, interleave_, loop_start=-1, loop_end=None, coef_type=0, header_size=0x200,
               audio_offset=0x200):
    """A GENH file as GenhReader.ReadHeader reads it (the layout of the tools that write GENH: little-endian header,
    coefficients at absolute offsets in the byte order CoefType names, Split = 8 even + 8 odd shorts)."""
    nch = len(adpcm)
    n = len(adpcm[0])
    loop_end = nibble_count_to_sample_count(2 * n) if loop_end is None else loop_end
    coef_at = [0x40 + 0x40 * c for c in range(2)]
    split_at = [0x40 + 0x40 * c + 0x20 for c in range(2)]
    body = interleave([bytes(a) for a in adpcm], interleave_, n) if nch > 1 else bytes(adpcm[0])
    out = bytearray(max(audio_offset, 0x100) + len(body))
    struct.pack_into("<4s14i", out, 0, b"GENH", nch, interleave_, sample_rate, loop_start, loop_end, 12, audio_offset,
                     header_size, coef_at[0], coef_at[1], 0, coef_type, split_at[0], split_at[1])
    e = "<" if coef_type & 2 else ">"
    for c in range(nch):
        if coef_type & 1:
            struct.pack_into(e + "8h", out, coef_at[c], *coefs[c][0::2])
            struct.pack_into(e + "8h", out, split_at[c], *coefs[c][1::2])
        else:
            struct.pack_into(e + "16h", out, coef_at[c], *coefs[c])
    out[audio_offset:audio_offset + len(body)] = body
    return bytes(out)


def genh_parse(data):
    """GenhReader.ReadFile"""
    if data[:4] != b"GENH":
        raise ValueError("magic")
    v = struct.unpack_from("<14i", data, 4)
    nch, il, rate, ls, le, codec, ado, hs, c0, c1, it, ct, s0, s1 = v
    if nch < 1 or nch > 2 or hs > ado:
        raise ValueError("header")
    e = "<" if ct & 2 else ">"
    coefs = []
    for c, (at, sp) in enumerate(((c0, s0), (c1, s1))[:nch]):
        if ct & 1:
            even, odd = struct.unpack_from(e + "8h", data, at), struct.unpack_from(e + "8h", data, sp)
            coefs.append([x for pair in zip(even, odd) for x in pair])
        else:
            coefs.append(list(struct.unpack_from(e + "16h", data, at)))
    sc = le
    audio = deinterleave(data[ado:], bytes_of(sc) * nch, il, nch)
    return dict(channel_count=nch, interleave=il, sample_rate=rate, loop_start=ls, loop_end=le, sample_count=sc,
                looping=ls != -1, coefs=coefs, audio=audio, audio_data_offset=ado, header_size=hs, coef_type=ct)
