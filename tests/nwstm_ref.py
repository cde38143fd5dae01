"""An independent restatement of the NintendoWare stream containers for the tests (not imported by the product).

build_image() follows BrstmWriter.cs / BCFstmWriter.cs line by line with `struct`; parse_image() reads an image the
way docs/010-editor-templates/brstm.bt and bfstm.bt lay the formats out (block table -> INFO/HEAD references ->
stream info, track table, channel table), not the way the reference readers do, so the writer and the parser under
test are not checked against one shared reading."""
import struct

DEFAULT = 14336


def bytes_of(n):                                  # GcAdpcmMath.SampleCountToByteCount
    frames, rem = divmod(n, 14)
    return frames * 8 + (0 if rem == 0 else 1 + (rem + 1) // 2)


def next_multiple(v, m):
    return v if m == 0 or v % m == 0 else v + m - v % m


def div_up(v, d):
    return -(-v // d)


def flags(target, version):
    """Common.cs:103-135 -> (track info, region info, unaligned loop)"""
    major = version >> 24
    track = (major == 0 and version <= 0x00020000) or (major >= 2 and version <= 0x02010000)
    region = (major >= 2 and version >= 0x02010000) or major == 0
    unaligned = (major == 0 and version >= 0x00040000) or (major >= 2 and version >= 0x02030000)
    return track, region, unaligned


def default_tracks(nch):
    return [dict(channel_count=min(nch - 2 * i, 2), left=2 * i, right=2 * i + 1 if nch - 2 * i >= 2 else 0,
                 volume=0x7f, panning=0x40) for i in range(div_up(nch, 2))]


def layout(target, nch, sample_count, looping=False, loop_start=0, loop_end=0, spi=DEFAULT, spe=DEFAULT,
           track_short=False, seek_short=False, version=None, ntracks=None):
    """the derived quantities of BrstmWriter.cs:22-74 / BCFstmWriter.cs:23-83 for an already aligned format"""
    T = div_up(nch, 2) if ntracks is None else ntracks
    sc = loop_end if looping else sample_count
    d = dict(sample_count=sc)
    d["audio_data_size"] = next_multiple(bytes_of(sc), 0x20)
    d["interleave_size"] = bytes_of(spi)
    d["interleave_count"] = div_up(sc, spi)
    d["last_block_samples"] = sc - (d["interleave_count"] - 1) * spi
    d["last_block_size_without_padding"] = bytes_of(d["last_block_samples"])
    d["last_block_size"] = next_multiple(d["last_block_size_without_padding"], 0x20)
    if target == 0:
        d["seek_table_entry_count"] = bytes_of(sc) // spe + 1 if seek_short else div_up(sc, spe)
        h1, h2 = 0x34, 4 + 8 * T + (4 if track_short else 0x0c) * T
        h3 = 4 + 8 * nch + 0x38 * nch
    else:
        if version is None:
            version = 0x02010000 if target == 1 else 0x00030000
        track, region, unaligned = flags(target, version)
        d["seek_table_entry_count"] = div_up(sc, spe)
        h1 = 0x38 + (0xc if region else 0) + (8 if unaligned else 0)
        h2 = 4 + 8 * T if track else 0
        h3 = 4 + 8 * nch + (0x14 * T if track else 0) + 8 * nch + 0x2e * nch
    d["h1"], d["h2"], d["h3"] = h1, h2, h3
    d["head_block_size"] = next_multiple(8 + 24 + h1 + h2 + h3, 0x20)
    d["seek_block_size"] = next_multiple(8 + d["seek_table_entry_count"] * nch * 4, 0x20)
    d["data_block_offset"] = 0x40 + d["head_block_size"] + d["seek_block_size"]
    d["data_block_size"] = 0x20 + d["audio_data_size"] * nch
    d["audio_data_offset"] = d["data_block_offset"] + 0x20
    d["file_size"] = 0x40 + d["head_block_size"] + d["seek_block_size"] + d["data_block_size"]
    return d


class W:
    """BinaryWriter over MemoryStream(byte[FileSize])"""

    def __init__(self, size, big):
        self.b, self.pos, self.e = bytearray(size), 0, ">" if big else "<"

    def raw(self, data):
        self.b[self.pos:self.pos + len(data)] = data
        self.pos += len(data)

    def u8(self, v):
        self.raw(struct.pack("B", v & 0xff))

    def i16(self, v):
        self.raw(struct.pack(self.e + "H", v & 0xffff))

    def i32(self, v):
        self.raw(struct.pack(self.e + "I", v & 0xffffffff))


def build_image(target, sample_rate, nch, adpcm, coefs, gain, start, loopctx, seek, looping, loop_start, loop_end,
                sample_count, spi=DEFAULT, spe=DEFAULT, track_short=False, seek_short=False, version=None, big=None,
                tracks=None):
    """adpcm: nch byte strings (GetAdpcmAudio, after alignment); coefs nch x 16; gain nch; start / loopctx nch x 3;
    seek: nch lists of the builder's seek table shorts; loop points and sample_count of the aligned format."""
    tracks = default_tracks(nch) if tracks is None else tracks
    T = len(tracks)
    L = layout(target, nch, sample_count, looping, loop_start, loop_end, spi, spe, track_short, seek_short, version, T)
    sc = L["sample_count"]
    if target != 0 and version is None:
        version = 0x02010000 if target == 1 else 0x00030000
    if big is None:
        big = target != 1
    w = W(L["file_size"], True if target == 0 else big)
    head, seekb = L["head_block_size"], L["seek_block_size"]
    seek_off, data_off = 0x40 + head, 0x40 + head + seekb
    ctx_loop = [loopctx[c] if looping else start[c] for c in range(nch)]

    def ctx(v):
        for x in v:
            w.i16(x)

    if target == 0:
        w.raw(b"RSTM"); w.i16(0xfeff); w.i16(0x0100); w.i32(L["file_size"]); w.i16(0x40); w.i16(2)
        w.i32(0x40); w.i32(head); w.i32(seek_off); w.i32(seekb); w.i32(data_off); w.i32(L["data_block_size"])
        w.pos = 0x40
        w.raw(b"HEAD"); w.i32(head)
        w.i32(0x01000000); w.i32(24); w.i32(0x01000000); w.i32(24 + 0x34); w.i32(0x01000000); w.i32(24 + 0x34 + L["h2"])
        w.u8(2); w.u8(int(looping)); w.u8(nch); w.u8(0); w.i16(sample_rate); w.i16(0)
        w.i32(loop_start); w.i32(sc); w.i32(L["audio_data_offset"]); w.i32(L["interleave_count"])
        w.i32(L["interleave_size"]); w.i32(spi); w.i32(L["last_block_size_without_padding"])
        w.i32(L["last_block_samples"]); w.i32(L["last_block_size"]); w.i32(spe); w.i32(4)
        w.u8(T); w.u8(0 if track_short else 1); w.i16(0)
        tis = 4 if track_short else 0x0c
        base = 24 + 0x34 + 4
        for i in range(T):
            w.i32(0x01000000 if track_short else 0x01010000); w.i32(base + T * 8 + tis * i)
        for t in tracks:
            if not track_short:
                w.u8(t["volume"]); w.u8(t["panning"]); w.i16(0); w.i32(0)
            w.u8(t["channel_count"]); w.u8(t["left"]); w.u8(t["right"]); w.u8(0)
        w.u8(nch); w.u8(0); w.i16(0)
        base = 24 + 0x34 + L["h2"] + 4
        for i in range(nch):
            w.i32(0x01000000); w.i32(base + nch * 8 + 0x38 * i)
        for i in range(nch):
            w.i32(0x01000000); w.i32(base + nch * 8 + 0x38 * i + 8)
            ctx(coefs[i]); w.i16(gain[i]); ctx(start[i]); ctx(ctx_loop[i]); w.i16(0)
        w.pos = seek_off
        w.raw(b"ADPC"); w.i32(seekb)
        table_big = True
    else:
        track, region, unaligned = flags(target, version)
        word = (4 if unaligned else 3) if target == 2 else (0x201 if track and region else 0x202 if region else 0x200)
        w.raw(b"CSTM" if target == 1 else b"FSTM"); w.i16(0xfeff); w.i16(0x40); w.i32(word << 16); w.i32(L["file_size"])
        w.i16(3); w.i16(0)
        for typ, off, size in ((0x4000, 0x40, head), (0x4001, seek_off, seekb), (0x4002, data_off, L["data_block_size"])):
            w.i16(typ); w.i16(0); w.i32(off); w.i32(size)
        w.pos = 0x40
        w.raw(b"INFO"); w.i32(head)
        w.i16(0x4100); w.i16(0); w.i32(24)
        if track:
            w.i16(0x0101); w.i16(0); w.i32(24 + L["h1"])
        else:
            w.i32(0); w.i32(-1)
        w.i16(0x0101); w.i16(0); w.i32(24 + L["h1"] + L["h2"])
        w.u8(2); w.u8(int(looping)); w.u8(nch); w.u8(0); w.i32(sample_rate); w.i32(loop_start); w.i32(sc)
        w.i32(L["interleave_count"]); w.i32(L["interleave_size"]); w.i32(spi); w.i32(L["last_block_size_without_padding"])
        w.i32(L["last_block_samples"]); w.i32(L["last_block_size"]); w.i32(4); w.i32(spe)
        w.i16(0x1F00); w.i16(0); w.i32(0x18)
        if region:
            w.i16(0x0100); w.i16(0); w.i32(0); w.i32(-1)
        if unaligned:
            w.i32(loop_start); w.i32(loop_end)
        if track:
            w.i32(T)
            for i in range(T):
                w.i16(0x4101); w.i16(0); w.i32(4 + 8 * T + 4 + 8 * nch + 0x14 * i)
        tts = 0x14 * T if track else 0
        w.i32(nch)
        for i in range(nch):
            w.i16(0x4102); w.i16(0); w.i32(4 + 8 * nch + tts + 8 * i)
        if track:
            for t in tracks:
                w.u8(t["volume"]); w.u8(t["panning"]); w.i16(0); w.i16(0x0100); w.i16(0); w.i32(0xc)
                w.i32(t["channel_count"]); w.u8(t["left"]); w.u8(t["right"]); w.i16(0)
        for i in range(nch):
            w.i16(0x0300); w.i16(0); w.i32(8 * nch - 8 * i + 0x2e * i)
        for i in range(nch):
            ctx(coefs[i]); ctx(start[i]); ctx(ctx_loop[i]); w.i16(0)
        w.pos = seek_off
        w.raw(b"SEEK"); w.i32(seekb)
        table_big = False                                        # BCFstmWriter.cs:340
    n = L["seek_table_entry_count"]
    inter = [0] * (n * 2 * nch)
    for c in range(nch):
        for e in range(min(n, len(seek[c]) // 2)):
            inter[e * 2 * nch + 2 * c:e * 2 * nch + 2 * c + 2] = seek[c][2 * e:2 * e + 2]
    w.raw(struct.pack((">" if table_big else "<") + "%dh" % len(inter), *inter))
    w.pos = data_off
    w.raw(b"DATA"); w.i32(L["data_block_size"])
    if target == 0:
        w.i32(0x18)
    # Interleave(channels, InterleaveSize, AudioDataSize)
    isz, osz = L["interleave_size"], L["audio_data_size"]
    insz = len(adpcm[0]) if nch else 0
    inb, outb = div_up(insz, isz), div_up(osz, isz)
    pos = L["audio_data_offset"]
    for b in range(min(inb, outb)):
        ci = insz - (inb - 1) * isz if b == inb - 1 else isz
        co = osz - (outb - 1) * isz if b == outb - 1 else isz
        k = min(ci, co)
        for c in range(nch):
            w.b[pos:pos + k] = adpcm[c][isz * b:isz * b + k]
            pos += co
    return bytes(w.b)


class R:
    def __init__(self, data, big):
        self.d, self.e = data, ">" if big else "<"

    def u8(self, o):
        return self.d[o]

    def u16(self, o):
        return struct.unpack_from(self.e + "H", self.d, o)[0]

    def s16(self, o):
        return struct.unpack_from(self.e + "h", self.d, o)[0]

    def s32(self, o):
        return struct.unpack_from(self.e + "i", self.d, o)[0]


def parse_image(data):
    """-> dict: header fields, tracks, per-channel coefs/gain/contexts, seek tables and de-interleaved audio"""
    magic = data[:4]
    out = dict(magic=magic)
    if magic == b"RSTM":
        r = R(data, True)
        out.update(target=0, big=True, file_size=r.s32(8))
        head_off, seek_off, seek_size, data_off, data_size = r.s32(0x10), r.s32(0x18), r.s32(0x1c), r.s32(0x20), r.s32(0x24)
        base = head_off + 8
        si, ti, ci = (base + r.s32(base + 4 + 8 * k) for k in range(3))
        out.update(codec=r.u8(si), looping=r.u8(si + 1), nch=r.u8(si + 2), sample_rate=r.u16(si + 4),
                   loop_start=r.s32(si + 8), sample_count=r.s32(si + 12), audio_offset=r.s32(si + 16),
                   interleave_count=r.s32(si + 20), interleave_size=r.s32(si + 24), spi=r.s32(si + 28),
                   lbs_nopad=r.s32(si + 32), lb_samples=r.s32(si + 36), lbs=r.s32(si + 40), spe=r.s32(si + 44))
        T, standard = r.u8(ti), r.u8(ti + 1)
        tracks = []
        for i in range(T):
            t = base + r.s32(ti + 4 + 8 * i + 4)
            if standard:
                tracks.append(dict(volume=r.u8(t), panning=r.u8(t + 1), channel_count=r.u8(t + 8), left=r.u8(t + 9),
                                   right=r.u8(t + 10)))
            else:
                tracks.append(dict(volume=0x7f, panning=0x40, channel_count=r.u8(t), left=r.u8(t + 1), right=r.u8(t + 2)))
        nch = out["nch"]
        chans = []
        for i in range(nch):
            c = base + r.s32(ci + 4 + 8 * i + 4)
            a = base + r.s32(c + 4)
            chans.append(dict(coefs=[r.s16(a + 2 * k) for k in range(16)], gain=r.s16(a + 32),
                              start=[r.s16(a + 34 + 2 * k) for k in range(3)], loop=[r.s16(a + 40 + 2 * k) for k in range(3)]))
        table_e, table_off, table_bytes = ">", seek_off + 8, seek_size - 8
        audio_off = out["audio_offset"]
        audio_len = data_size - (audio_off - data_off)
        out["track_short"] = not standard
    else:
        big = data[4:6] == b"\xfe\xff"
        r = R(data, big)
        out.update(target=1 if magic == b"CSTM" else 2, big=big, version=r.s32(8) & 0xffffffff, file_size=r.s32(12))
        blocks = {}
        for k in range(r.u16(16)):
            o = 20 + 12 * k
            blocks[r.u16(o)] = (r.s32(o + 4), r.s32(o + 8))
        info_off = blocks[0x4000][0]
        base = info_off + 8
        refs = [(r.u16(base + 8 * k), r.s32(base + 8 * k + 4)) for k in range(3)]
        si = base + refs[0][1]
        out.update(codec=r.u8(si), looping=r.u8(si + 1), nch=r.u8(si + 2), sample_rate=r.s32(si + 4),
                   loop_start=r.s32(si + 8), sample_count=r.s32(si + 12), interleave_count=r.s32(si + 16),
                   interleave_size=r.s32(si + 20), spi=r.s32(si + 24), lbs_nopad=r.s32(si + 28), lb_samples=r.s32(si + 32),
                   lbs=r.s32(si + 36), spe=r.s32(si + 44))
        audio_ref = r.s32(si + 52)
        tracks = []
        if refs[1][0] == 0x0101:
            tt = base + refs[1][1]
            for i in range(r.s32(tt)):
                t = tt + r.s32(tt + 4 + 8 * i + 4)
                cc = t + r.s32(t + 8)
                tracks.append(dict(volume=r.u8(t), panning=r.u8(t + 1), channel_count=r.s32(cc), left=r.u8(cc + 4),
                                   right=r.u8(cc + 5)))
        ct = base + refs[2][1]
        nch = out["nch"]
        chans = []
        for i in range(r.s32(ct)):
            c = ct + r.s32(ct + 4 + 8 * i + 4)
            a = c + r.s32(c + 4)
            chans.append(dict(coefs=[r.s16(a + 2 * k) for k in range(16)], gain=0,
                              start=[r.s16(a + 32 + 2 * k) for k in range(3)], loop=[r.s16(a + 38 + 2 * k) for k in range(3)]))
        seek_off, seek_size = blocks[0x4001]
        data_off, data_size = blocks[0x4002]
        table_e, table_off, table_bytes = "<", seek_off + 8, seek_size - 8
        audio_off = data_off + 8 + audio_ref
        audio_len = data_size - (audio_off - data_off)
    out["tracks"], out["channels"] = tracks, chans
    entries = table_bytes // (4 * nch)
    table = struct.unpack_from(table_e + "%dh" % (entries * 2 * nch), data, table_off)
    out["seek_raw"] = [[v for e in range(entries) for v in table[e * 2 * nch + 2 * c:e * 2 * nch + 2 * c + 2]]
                       for c in range(nch)]
    # DeInterleave(length, InterleaveSize, ChannelCount, SampleCountToByteCount(SampleCount))
    isz, insz, osz = out["interleave_size"], audio_len // nch, bytes_of(out["sample_count"])
    inb, outb = div_up(insz, isz), div_up(osz, isz)
    chans_audio = [bytearray(osz) for _ in range(nch)]
    for b in range(min(inb, outb)):
        ci = insz - (inb - 1) * isz if b == inb - 1 else isz
        co = osz - (outb - 1) * isz if b == outb - 1 else isz
        k = min(ci, co)
        for o in range(nch):
            s = audio_off + isz * b * nch + ci * o
            chans_audio[o][isz * b:isz * b + k] = data[s:s + k]
    out["audio"] = [bytes(a) for a in chans_audio]
    out["audio_offset"], out["audio_length"] = audio_off, audio_len
    return out
