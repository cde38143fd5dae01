"""Independent restatement of the PCM8 / PCM16 branches of BrstmWriter.cs and BCFstmWriter.cs (line by line, with
struct) and a parser laid out as docs/010-editor-templates/brstm.bt and bfstm.bt -- for the tests only."""
import struct

import numpy as np

from nwstm_ref import R, W, default_tracks, div_up, flags, next_multiple

PCM8, PCM16 = 0, 1
RSTM, CSTM, FSTM = 0, 1, 2
MARKER, MARKER_V2 = 0x01000000, 0x01010000


def bps(codec):
    return 2 if codec == PCM16 else 1


def default_samples(codec):                       # BytesToSamples(0x2000, codec)
    return 0x2000 // bps(codec)


def encode_signed(s16):                          # Pcm8Codec.EncodeSigned
    return (np.asarray(s16, dtype=np.int16) >> 8).astype(np.int8).view(np.uint8)


def decode_signed(b):                            # Pcm8Codec.DecodeSigned
    return (np.asarray(b, dtype=np.uint8).view(np.int8).astype(np.int16) << 8).astype(np.int16)


def layout(target, codec, nch, sample_count, looping=False, loop_start=0, loop_end=0, spi=None, spe=None,
           track_short=False, version=None, ntracks=None):
    """every size and offset of the writer, as a dict (the names of vga_nwstm_layout)"""
    k = bps(codec)
    spi = spi or default_samples(codec)
    spe = spe or default_samples(codec)
    sc = loop_end if looping else sample_count
    T = ntracks if ntracks is not None else div_up(nch, 2)
    L = dict(sample_count=sc, track_count=T, samples_per_interleave=spi, interleave_size=spi * k)
    L["interleave_count"] = div_up(sc, spi)
    L["last_block_samples"] = sc - (L["interleave_count"] - 1) * spi
    L["last_block_size_without_padding"] = L["last_block_samples"] * k
    L["last_block_size"] = next_multiple(L["last_block_size_without_padding"], 0x20)
    L["audio_data_size"] = next_multiple(sc * k, 0x20)
    if target == RSTM:
        L.update(samples_per_seek_table_entry=0, bytes_per_seek_table_entry=0, head1_size=0x34,
                 head2_size=4 + 8 * T + (4 if track_short else 0x0c) * T, head3_size=4 + 8 * nch + 8 * nch)
        L.update(include_track_info=0, include_region_info=0, include_unaligned_loop=0)
    else:
        v = version or (0x02010000 if target == CSTM else 0x00030000)
        track, region, unaligned = flags(target, v)
        L.update(samples_per_seek_table_entry=spe, bytes_per_seek_table_entry=4,
                 head1_size=0x38 + (0xc if region else 0) + (8 if unaligned else 0),
                 head2_size=4 + 8 * T if track else 0,
                 head3_size=4 + 8 * nch + (0x14 * T if track else 0) + 8 * nch)
        L.update(include_track_info=int(track), include_region_info=int(region), include_unaligned_loop=int(unaligned))
        L["version_word"] = ((4 if unaligned else 3) if target == FSTM else
                             0x201 if track and region else 0x202 if region else 0x200) << 16
    L["head_block_offset"] = 0x40
    L["head_block_size"] = next_multiple(8 + 24 + L["head1_size"] + L["head2_size"] + L["head3_size"], 0x20)
    L["seek_block_offset"] = L["seek_block_size"] = 0
    L["data_block_offset"] = 0x40 + L["head_block_size"]
    L["data_block_size"] = 0x20 + L["audio_data_size"] * nch
    L["audio_data_offset"] = L["data_block_offset"] + 0x20
    L["file_size"] = 0x40 + L["head_block_size"] + L["data_block_size"]
    return L


def channel_bytes(codec, row, big):
    """Pcm16.Channels[c].ToByteArray(endianness) / Pcm8.Channels[c] (signed bytes)"""
    if codec == PCM16:
        return np.asarray(row, dtype=">i2" if big else "<i2").tobytes()
    return bytes(np.asarray(row, dtype=np.uint8))


def interleave(chans, isz, out_size):
    """Interleave(Stream, interleaveSize, outputSize) (Interleave.cs:43-78) into a fresh zeroed buffer"""
    n_in = len(chans[0])
    inb, outb = div_up(n_in, isz), div_up(out_size, isz)
    last_in, last_out = n_in - (inb - 1) * isz, out_size - (outb - 1) * isz
    out = bytearray(out_size * len(chans))
    pos = 0
    for b in range(min(inb, outb)):
        ci = last_in if b == inb - 1 else isz
        co = last_out if b == outb - 1 else isz
        k = min(ci, co)
        for c in chans:
            out[pos:pos + k] = c[isz * b:isz * b + k]
            pos += co
    return bytes(out)


def build_image(target, codec, sample_rate, rows, looping=False, loop_start=0, loop_end=0, spi=None, spe=None,
                track_short=False, version=None, big=None, tracks=None):
    """the writer's bytes for rows as stored (int16 for PCM16, signed bytes for PCM8)"""
    nch = len(rows)
    tracks = tracks if tracks is not None else default_tracks(nch)
    T = len(tracks)
    L = layout(target, codec, nch, len(rows[0]), looping, loop_start, loop_end, spi, spe, track_short, version, T)
    if target == RSTM:
        big = True
    elif big is None:
        big = target == FSTM
    w = W(L["file_size"], big)
    if target == RSTM:
        w.raw(b"RSTM"); w.i16(0xfeff); w.i16(0x0100); w.i32(L["file_size"]); w.i16(0x40); w.i16(2)
        w.i32(0x40); w.i32(L["head_block_size"]); w.i32(0); w.i32(0); w.i32(L["data_block_offset"]); w.i32(L["data_block_size"])
        w.pos = 0x40
        w.raw(b"HEAD"); w.i32(L["head_block_size"])
        w.i32(MARKER); w.i32(24); w.i32(MARKER); w.i32(24 + 0x34); w.i32(MARKER); w.i32(24 + 0x34 + L["head2_size"])
        w.u8(codec); w.u8(int(looping)); w.u8(nch); w.u8(0); w.i16(sample_rate); w.i16(0)
        w.i32(loop_start if looping else 0); w.i32(L["sample_count"]); w.i32(L["audio_data_offset"])
        for key in ("interleave_count", "interleave_size", "samples_per_interleave", "last_block_size_without_padding",
                    "last_block_samples", "last_block_size"):
            w.i32(L[key])
        w.i32(0); w.i32(0)                        # SamplesPerSeekTableEntry, BytesPerSeekTableEntry
        tsize = 4 if track_short else 0x0c
        w.u8(T); w.u8(0 if track_short else 1); w.i16(0)
        for i in range(T):
            w.i32(MARKER if track_short else MARKER_V2); w.i32(24 + 0x34 + 4 + 8 * T + tsize * i)
        for t in tracks:
            if not track_short:
                w.u8(t["volume"]); w.u8(t["panning"]); w.i16(0); w.i32(0)
            w.u8(t["channel_count"]); w.u8(t["left"]); w.u8(t["right"]); w.u8(0)
        w.u8(nch); w.u8(0); w.i16(0)
        base = 24 + 0x34 + L["head2_size"] + 4
        for i in range(nch):
            w.i32(MARKER); w.i32(base + 8 * nch + 8 * i)
        for i in range(nch):
            w.i32(MARKER); w.i32(0)
        w.pos = L["data_block_offset"]
        w.raw(b"DATA"); w.i32(L["data_block_size"]); w.i32(0x18)
    else:
        w.raw(b"CSTM" if target == CSTM else b"FSTM"); w.i16(0xfeff); w.i16(0x40); w.i32(L["version_word"])
        w.i32(L["file_size"]); w.i16(2); w.i16(0)
        w.i16(0x4000); w.i16(0); w.i32(0x40); w.i32(L["head_block_size"])
        w.i16(0x4002); w.i16(0); w.i32(L["data_block_offset"]); w.i32(L["data_block_size"])
        w.pos = 0x40
        w.raw(b"INFO"); w.i32(L["head_block_size"])
        w.i16(0x4100); w.i16(0); w.i32(24)
        if L["include_track_info"]:
            w.i16(0x0101); w.i16(0); w.i32(24 + L["head1_size"])
        else:
            w.i32(0); w.i32(-1)
        w.i16(0x0101); w.i16(0); w.i32(24 + L["head1_size"] + L["head2_size"])
        w.u8(codec); w.u8(int(looping)); w.u8(nch); w.u8(0); w.i32(sample_rate)
        w.i32(loop_start if looping else 0); w.i32(L["sample_count"])
        for key in ("interleave_count", "interleave_size", "samples_per_interleave", "last_block_size_without_padding",
                    "last_block_samples", "last_block_size"):
            w.i32(L[key])
        w.i32(4); w.i32(L["samples_per_seek_table_entry"])
        w.i16(0x1F00); w.i16(0); w.i32(0x18)
        if L["include_region_info"]:
            w.i16(0x0100); w.i16(0); w.i32(0); w.i32(-1)
        if L["include_track_info"]:
            w.i32(T)
            for i in range(T):
                w.i16(0x4101); w.i16(0); w.i32(4 + 8 * T + 4 + 8 * nch + 0x14 * i)
        w.i32(nch)
        tts = 0x14 * T if L["include_track_info"] else 0
        for i in range(nch):
            w.i16(0x4102); w.i16(0); w.i32(4 + 8 * nch + tts + 8 * i)
        if L["include_track_info"]:
            for t in tracks:
                w.u8(t["volume"]); w.u8(t["panning"]); w.i16(0); w.i16(0x0100); w.i16(0); w.i32(0xc)
                w.i32(t["channel_count"]); w.u8(t["left"]); w.u8(t["right"]); w.i16(0)
        for i in range(nch):
            w.i32(0); w.i32(-1)
        w.pos = L["data_block_offset"]
        w.raw(b"DATA"); w.i32(L["data_block_size"])
    chans = [channel_bytes(codec, r, big) for r in rows]
    audio = interleave(chans, L["interleave_size"], L["audio_data_size"])
    w.b[L["audio_data_offset"]:L["audio_data_offset"] + len(audio)] = audio
    return bytes(w.b)


def parse_image(data):
    """-> dict of the stream info, tracks and the de-interleaved channels (int16 for PCM16, uint8 for PCM8)"""
    magic = bytes(data[:4])
    out = dict(magic=magic)
    if magic == b"RSTM":
        r = R(data, True)
        big = True
        data_off, data_size = r.s32(0x20), r.s32(0x24)
        base = r.s32(0x10) + 8
        si, ti = base + r.s32(base + 4), base + r.s32(base + 12)
        out.update(codec=r.u8(si), looping=r.u8(si + 1), nch=r.u8(si + 2), sample_rate=r.u16(si + 4),
                   loop_start=r.s32(si + 8), sample_count=r.s32(si + 12), audio_offset=r.s32(si + 16),
                   interleave_size=r.s32(si + 24), spe=r.s32(si + 44), bpe=r.s32(si + 48),
                   seek_offset=r.s32(0x18), seek_size=r.s32(0x1c))
        T, standard = r.u8(ti), r.u8(ti + 1)
        tracks = []
        for i in range(T):
            o = base + r.s32(ti + 4 + 8 * i + 4)
            t = dict(volume=0x7f, panning=0x40)
            if standard:
                t.update(volume=r.u8(o), panning=r.u8(o + 1))
                o += 8
            t.update(channel_count=r.u8(o), left=r.u8(o + 1), right=r.u8(o + 2))
            tracks.append(t)
        out["tracks"] = tracks
    else:
        big = struct.unpack_from("<H", data, 4)[0] == 0xFFFE
        r = R(data, big)
        out["nblocks"] = r.u16(0x10)
        blocks = {r.u16(0x14 + 12 * i): (r.s32(0x18 + 12 * i), r.s32(0x1c + 12 * i)) for i in range(out["nblocks"])}
        info = blocks[0x4000][0]
        data_off, data_size = blocks[0x4002]
        base = info + 8
        si = base + r.s32(base + 4)
        out.update(codec=r.u8(si), looping=r.u8(si + 1), nch=r.u8(si + 2), sample_rate=r.s32(si + 4),
                   loop_start=r.s32(si + 8), sample_count=r.s32(si + 12), interleave_size=r.s32(si + 20),
                   bpe=r.s32(si + 40), spe=r.s32(si + 44), audio_offset=data_off + 8 + r.s32(si + 52))
        tracks = []
        if r.s32(base + 12) != -1:
            tb = base + r.s32(base + 12)
            for i in range(r.s32(tb)):
                o = tb + r.s32(tb + 4 + 8 * i + 4)
                cc = o + r.s32(o + 8)
                tracks.append(dict(volume=r.u8(o), panning=r.u8(o + 1), channel_count=r.s32(cc), left=r.u8(cc + 4),
                                   right=r.u8(cc + 5)))
        out["tracks"] = tracks
    out["big"] = big
    nch, k = out["nch"], bps(out["codec"])
    length = data_size - (out["audio_offset"] - data_off)
    per, isz, size = length // nch, out["interleave_size"], out["sample_count"] * k
    inb, outb = div_up(per, isz), div_up(size, isz)
    last_in, last_out = per - (inb - 1) * isz, size - (outb - 1) * isz
    chans = [bytearray(size) for _ in range(nch)]
    for b in range(min(inb, outb)):
        ci = last_in if b == inb - 1 else isz
        co = last_out if b == outb - 1 else isz
        n = min(ci, co)
        for c in range(nch):
            src = out["audio_offset"] + isz * b * nch + ci * c
            chans[c][isz * b:isz * b + n] = data[src:src + n]
    if out["codec"] == PCM16:
        out["channels"] = [np.frombuffer(bytes(c), dtype=">i2" if big else "<i2").astype(np.int16) for c in chans]
    else:
        out["channels"] = [np.frombuffer(bytes(c), dtype=np.uint8).copy() for c in chans]
    return out
