"""NintendoWare wave files (RWAV, CWAV, FWAV) and prefetch files (CSTP, FSTP) for the tests, not imported by the product
and not calling it.  The reference writes none of these formats, so two independent things live here, both restated
from its C# readers:

  build_rwav / build_bcfwav / build_prefetch   lay out an image from given channels (field offsets as
      BrwavReader.cs, RwavWaveInfo.cs, RwavChannelInfo.cs, BCFstmReader.cs, StreamInfo.cs, ChannelInfo.cs and
      PrefetchData.cs read them);
  read_image   BrwavReader.ReadFile / BCFstmReader.ReadFile followed by Common.ToAudioStream's bookkeeping: the
      structure's fields and each channel's stored bytes."""
import struct

PCM8, PCM16, GCADPCM = 0, 1, 2
RWAV, CWAV, FWAV, CSTP, FSTP = range(5)
MAGIC = {RWAV: b"RWAV", CWAV: b"CWAV", FWAV: b"FWAV", CSTP: b"CSTP", FSTP: b"FSTP"}


class Invalid(Exception):
    """InvalidDataException"""


def cdiv(a, b):                                   # C# integer division
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def crem(a, b):
    return a - b * cdiv(a, b)


def nibble_to_sample(n):                          # GcAdpcmMath.NibbleToSample
    return 14 * cdiv(n, 16) + crem(n, 16) - 2


def sample_to_nibble(s):                          # GcAdpcmMath.SampleToNibble
    return 16 * (s // 14) + s % 14 + 2


def samples_to_bytes(n, codec):                   # Common.SamplesToBytes
    if codec == GCADPCM:
        frames, extra = divmod(n, 14)
        return (16 * frames + (extra + 2 if extra else 0) + 1) // 2
    return n * 2 if codec == PCM16 else n if codec == PCM8 else 0


def bytes_to_samples(b, codec):                   # Common.BytesToSamples
    if codec == GCADPCM:
        frames, extra = divmod(b * 2, 16)
        return 14 * frames + (0 if extra < 2 else extra - 2)
    return b // 2 if codec == PCM16 else b if codec == PCM8 else 0


def unaligned_loop_wave(version):                 # Common.IncludeUnalignedLoopWave
    major = version >> 24
    return (major == 0 and version >= 0x00010200) or (major >= 2 and version >= 0x02010100)


def stream_flags(version):                        # Common.IncludeRegionInfo / IncludeUnalignedLoop / IncludeChecksum
    major = version >> 24
    return ((major >= 2 and version >= 0x02010000) or major == 0,
            (major == 0 and version >= 0x00040000) or (major >= 2 and version >= 0x02030000),
            major == 0 and version >= 0x00050000)


class W:
    def __init__(self, big):
        self.b, self.e = bytearray(), ">" if big else "<"

    @property
    def pos(self):
        return len(self.b)

    def raw(self, data):
        self.b += bytes(data)

    def u8(self, *vs):
        for v in vs:
            self.b += struct.pack("B", v & 0xff)

    def i16(self, *vs):
        for v in vs:
            self.b += struct.pack(self.e + "H", v & 0xffff)

    def i32(self, *vs):
        for v in vs:
            self.b += struct.pack(self.e + "I", v & 0xffffffff)

    def ref(self, typ, off):                      # Reference: type, 2 bytes, offset
        self.i16(typ, 0)
        self.i32(off)

    def patch32(self, at, v):
        self.b[at:at + 4] = struct.pack(self.e + "I", v & 0xffffffff)

    def pad_to(self, multiple, fill=0):
        while len(self.b) % multiple:
            self.b.append(fill)


def _place(w, base, audio, order, gaps, filler):
    """the channels' audio in `order`, gaps[i] filler bytes before the i-th placed -> offsets from `base` by channel"""
    offs = [0] * len(audio)
    for i, c in enumerate(order):
        w.raw(filler[:gaps[i]])
        offs[c] = w.pos - base
        w.raw(audio[c])
    return offs


def build_rwav(codec, sample_rate, sample_count, audio, infos=None, looping=False, loop_start=0, version=(1, 2), order=None,
               gaps=None, filler=b"\xa5" * 64, tail=0):
    """audio: per channel samples_to_bytes(sample_count, codec) bytes; infos: per channel (coefs16, gain, start3, loop3)"""
    nch = len(audio)
    order = list(range(nch)) if order is None else order
    gaps = [0] * nch if gaps is None else gaps
    infos = infos or [([0] * 16, 0, [0] * 3, [0] * 3)] * nch
    w = W(True)
    w.raw(b"RWAV"); w.i16(0xfeff); w.u8(*version); w.i32(0); w.i16(0x20, 2); w.i32(0x20, 0, 0, 0)
    w.raw(b"INFO"); w.i32(0)
    base = w.pos
    w.u8(codec, int(looping), nch, 0); w.i16(sample_rate, 0)
    w.i32(sample_to_nibble(loop_start), sample_to_nibble(sample_count), 0x18, 0)
    table = w.pos
    w.i32(*([0] * nch))
    chans = []
    for c in range(nch):
        w.patch32(table + 4 * c, w.pos - base)
        chans.append(w.pos)
        w.i32(0, 0, 0x01000000, 0x01000000, 0x01000000, 0x01000000, 0)
    for c in range(nch):
        coefs, gain, start, loop = infos[c]
        w.patch32(chans[c] + 4, w.pos - base)
        w.i16(*coefs); w.i16(gain); w.i16(*start); w.i16(*loop); w.i16(0)
    w.patch32(base + 0x14, w.pos - base)
    w.pad_to(0x20)
    info_size = w.pos - 0x20
    data_off = w.pos
    w.raw(b"DATA"); w.i32(0)
    offs = _place(w, w.pos, audio, order, gaps, filler)
    for c in range(nch):
        w.patch32(chans[c], offs[c])
    w.pad_to(0x20)
    w.raw(filler[:tail])
    w.patch32(8, w.pos)
    data_size = w.pos - tail - data_off
    w.patch32(0x14, info_size); w.patch32(0x18, data_off); w.patch32(0x1c, data_size)
    w.patch32(0x24, info_size); w.patch32(data_off + 4, data_size)
    return bytes(w.b)


def _bcf_header(w, kind, version, blocks):
    w.raw(MAGIC[kind]); w.i16(0xfeff); w.i16(0x40); w.i32(version); w.i32(0); w.i16(len(blocks), 0)
    at = w.pos
    for typ in blocks:
        w.ref(typ, 0); w.i32(0)
    w.pad_to(0x20)
    return at


def _adpcm_infos(w, infos, refs, bases):
    """the GC-ADPCM infos after the channel infos; refs[c]: where channel c's Reference sits, relative to bases[c]"""
    for c, (coefs, _gain, start, loop) in enumerate(infos):
        w.b[refs[c]:refs[c] + 8] = struct.pack(w.e + "HHI", 0x0300, 0, w.pos - bases[c])
        w.i16(*coefs); w.i16(*start); w.i16(*loop); w.i16(0)


def build_bcfwav(kind, big, version, codec, sample_rate, sample_count, audio, infos=None, looping=False, loop_start=0,
                 loop_start_unaligned=0, order=None, gaps=None, filler=b"\x5a" * 64, tail=0):
    nch = len(audio)
    order = list(range(nch)) if order is None else order
    gaps = [0] * nch if gaps is None else gaps
    w = W(big)
    blocks = _bcf_header(w, kind, version, [0x7000, 0x7001])
    info_off = w.pos
    w.raw(b"INFO"); w.i32(0)
    w.u8(codec, int(looping), 0, 0); w.i32(sample_rate, loop_start, sample_count)
    w.i32(loop_start_unaligned if unaligned_loop_wave(version) else 0)
    base = w.pos                                  # the reference table: ChannelInfo.ReadBfstm
    w.i32(nch)
    table = w.pos
    for _ in range(nch):
        w.ref(0x7100, 0)
    chans = []
    for c in range(nch):
        w.patch32(table + 8 * c + 4, w.pos - base)
        chans.append(w.pos)
        w.ref(0x1F00, 0)
        w.ref(0, -1)
        w.i32(0)
    if codec == GCADPCM:
        _adpcm_infos(w, infos, [p + 8 for p in chans], chans)
    w.pad_to(0x20)
    info_size = w.pos - info_off
    data_off = w.pos
    w.raw(b"DATA"); w.i32(0)
    offs = _place(w, w.pos, audio, order, gaps, filler)
    for c in range(nch):
        w.patch32(chans[c] + 4, offs[c])
    w.pad_to(0x20)
    data_size = w.pos - data_off
    w.raw(filler[:tail])
    w.patch32(0xc, w.pos)
    w.patch32(info_off + 4, info_size); w.patch32(data_off + 4, data_size)
    w.patch32(blocks + 4, info_off); w.patch32(blocks + 8, info_size)
    w.patch32(blocks + 16, data_off); w.patch32(blocks + 20, data_size)
    return bytes(w.b)


def interleave(channels, il):
    """the stream writers' layout with no padding: block b of every channel in turn, the last block short"""
    n = len(channels[0])
    out = bytearray()
    for at in range(0, n, il):
        for ch in channels:
            out += ch[at:at + il]
    return bytes(out)


def build_prefetch(kind, big, version, codec, sample_rate, regions, interleave_size, infos=None, nch=1, stream_looping=True,
                   stream_loop_start=0, stream_sample_count=1 << 20, gap=0, filler=b"\x3c" * 64):
    """regions: [(start_sample, [channel bytes, all of one length])]; each region's audio is interleave(channels)"""
    w = W(big)
    blocks = _bcf_header(w, kind, version, [0x4000, 0x4004])
    region, unaligned, checksum = stream_flags(version)
    info_off = w.pos
    w.raw(b"INFO"); w.i32(0)
    base = w.pos
    w.ref(0x4100, 24); w.ref(0, -1); w.ref(0x0101, 0)
    spi = bytes_to_samples(interleave_size, codec)
    w.u8(codec, int(stream_looping), nch, len(regions)); w.i32(sample_rate, stream_loop_start, stream_sample_count)
    w.i32(-(-stream_sample_count // max(spi, 1)), interleave_size, spi, interleave_size, spi, interleave_size, 4, spi)
    w.ref(0x1F00, 0x18)
    if region:
        w.i16(0x100, 0); w.ref(0, -1)
    if unaligned:
        w.i32(stream_loop_start, stream_sample_count)
    if checksum:
        w.i32(0x12345678)
    w.patch32(base + 20, w.pos - base)
    cbase = w.pos
    w.i32(nch)
    table = w.pos
    for _ in range(nch):
        w.ref(0x4102, 0)
    chans = []
    for c in range(nch):
        w.patch32(table + 8 * c + 4, w.pos - cbase)
        chans.append(w.pos)
        w.ref(0, -1)
    if codec == GCADPCM:
        _adpcm_infos(w, infos, chans, chans)
    w.pad_to(0x20)
    info_size = w.pos - info_off
    data_off = w.pos
    w.raw(b"PDAT"); w.i32(0); w.i32(len(regions))
    entries = []
    for start, chans_audio in regions:
        entries.append(w.pos)
        w.i32(start, len(chans_audio[0]) * nch, 0); w.ref(0x1F00, 0)
    w.raw(filler[:gap])
    for e, (_start, chans_audio) in zip(entries, regions):
        w.patch32(e + 16, w.pos - e)
        w.raw(interleave(chans_audio, interleave_size))
    w.pad_to(0x20)
    data_size = w.pos - data_off
    w.patch32(0xc, w.pos)
    w.patch32(info_off + 4, info_size); w.patch32(data_off + 4, data_size)
    w.patch32(blocks + 4, info_off); w.patch32(blocks + 8, info_size)
    w.patch32(blocks + 16, data_off); w.patch32(blocks + 20, data_size)
    return bytes(w.b)


# ---------------------------------------------------------------- the restated reader
class R:
    """BinaryReader / BinaryReaderBE over a MemoryStream"""

    def __init__(self, data, big):
        self.d, self.e, self.pos = bytes(data), ">" if big else "<", 0

    def _get(self, fmt, n):
        v = struct.unpack_from(self.e + fmt, self.d, self.pos)[0]
        self.pos += n
        return v

    def u8(self):
        return self._get("B", 1)

    def u16(self):
        return self._get("H", 2)

    def s16(self):
        return self._get("h", 2)

    def s32(self):
        return self._get("i", 4)

    def u32(self):
        return self._get("I", 4)

    def utf8(self, n):
        v = self.d[self.pos:self.pos + n]
        self.pos += n
        return v

    def read_bytes(self, n):                      # ReadBytes: short at the end of the stream
        return self.utf8(n)

    def ref(self, base=0):                        # Reference(reader, baseOffset) -> (type, offset, absolute)
        typ = self.s16()
        self.pos += 2
        off = self.s32()
        return typ, off, base + off


def _is(ref, typ):
    return ref[0] == typ and ref[1] > 0


def _gc_info(r, gain):
    coefs = [r.s16() for _ in range(16)]
    g = r.s16() if gain else 0
    return dict(coefs=coefs, gain=g, start=[r.s16() for _ in range(3)], loop=[r.s16() for _ in range(3)])


def _read_rwav(data):                             # BrwavReader.cs
    r = R(data, True)
    if r.utf8(4) != b"RWAV":
        raise Invalid("File has no RWAV header")
    bom = r.u16()
    if bom != 0xfeff:
        raise Invalid("Expected 65279, but got %d at offset 0x4" % bom)
    s = dict(kind=RWAV, big=True, version=r.u8() << 24 | r.u8() << 16, file_size=r.s32())
    if len(data) < s["file_size"]:
        raise Invalid("Actual file length is less than stated length")
    r.s16(); r.s16()
    head_off, head_size, data_off, data_size = r.s32(), r.s32(), r.s32(), r.s32()
    r.pos = head_off
    if r.utf8(4) != b"INFO":
        raise Invalid("Unknown or invalid INFO block")
    if r.s32() != head_size:
        raise Invalid("HEAD block size in RWAV header doesn't match size in HEAD header")
    base = r.pos
    s.update(codec=r.u8(), looping=r.u8() != 0, nch=r.u8())
    r.pos += 1
    s["sample_rate"] = r.u16()
    r.pos += 2
    s.update(loop_start=nibble_to_sample(r.s32()), sample_count=nibble_to_sample(r.s32()))
    table = r.s32()
    r.s32()
    r.pos = base + table
    offs = [r.s32() for _ in range(s["nch"])]
    chans, audio_offs = [], []
    for o in offs:
        r.pos = base + o
        audio_offs.append(r.s32())
        info_off = r.s32()
        r.pos = base + info_off
        chans.append(_gc_info(r, True))
    r.pos = data_off
    if r.utf8(4) != b"DATA":
        raise Invalid("Unknown or invalid DATA block")
    if r.s32() != data_size:
        raise Invalid("DATA block size in main header doesn't match size in DATA header")
    n = samples_to_bytes(s["sample_count"], s["codec"])
    base = r.pos
    s.update(channels=chans, audio_offsets=[base + o for o in audio_offs], audio=[data[base + o:base + o + n] for o in audio_offs])
    return s


def _channel_table(r):                            # ChannelInfo.ReadBfstm
    base = r.pos
    refs = [r.ref(base) for _ in range(r.s32())]
    waves, chans = [], []
    for ref in refs:
        r.pos = ref[2]
        if _is(ref, 0x7100):
            waves.append(r.ref()[1])
        ad = r.ref(ref[2])
        if _is(ad, 0x0300):
            r.pos = ad[2]
            chans.append(_gc_info(r, False))
    return len(refs), waves, chans


def _read_bcf(data):                              # BCFstmReader.cs
    if data[:4] not in (b"CSTM", b"FSTM", b"CWAV", b"FWAV", b"CSTP", b"FSTP"):
        raise Invalid("File has no CSTM or FSTM header")
    bom = struct.unpack_from("<H", data, 4)[0]
    if bom not in (0xFEFF, 0xFFFE):
        raise Invalid("File has no byte order mark")
    big = bom == 0xFFFE
    r = R(data, big)
    r.pos = 6
    r.s16()
    s = dict(big=big, version=r.u32(), file_size=r.s32())
    if len(data) < s["file_size"]:
        raise Invalid("Actual file length is less than stated length")
    nblocks = r.s16()
    r.pos += 2
    blocks = [r.ref() + (r.s32(),) for _ in range(nblocks)]
    info = next((b for b in blocks if b[0] in (0x4000, 0x7000)), None)
    if info is None:
        raise Invalid("File has no INFO block")
    r.pos = info[2]
    if r.utf8(4) != b"INFO":
        raise Invalid("Unknown or invalid INFO block")
    if r.s32() != info[3]:
        raise Invalid("INFO block size in main header doesn't match size in INFO header")
    if info[0] == 0x7000:                         # StreamInfo.ReadBfwav
        s.update(codec=r.u8(), looping=r.u8() != 0)
        r.pos += 2
        s.update(sample_rate=r.s32(), loop_start=r.s32(), sample_count=r.s32())
        if unaligned_loop_wave(s["version"]):
            s["loop_start_unaligned"] = r.s32()
        else:
            r.pos += 4
        s["nch"], waves, chans = _channel_table(r)
    else:
        base = r.pos
        si, _ti, ci = r.ref(base), r.ref(base), r.ref(base)
        if not _is(si, 0x4100):
            raise Invalid("Could not read stream info.")
        r.pos = si[2]                             # StreamInfo.ReadBfstm
        s.update(codec=r.u8(), looping=r.u8() != 0, nch=r.u8())
        r.u8()
        s.update(sample_rate=r.s32(), loop_start=r.s32(), sample_count=r.s32(), interleave_count=r.s32(), interleave_size=r.s32(),
                 samples_per_interleave=r.s32(), last_block_size_without_padding=r.s32(), last_block_samples=r.s32(),
                 last_block_size=r.s32())
        waves, chans = [], []
        if _is(ci, 0x0101):
            r.pos = ci[2]
            _n, waves, chans = _channel_table(r)
    s["channels"] = chans
    blk = next((b for b in blocks if b[0] in (0x4002, 0x4004, 0x7001)), None)
    if blk is None:
        raise Invalid("File has no DATA block")
    r.pos = blk[2]
    if r.utf8(4) not in (b"DATA", b"PDAT"):
        raise Invalid("Unknown or invalid DATA block")
    if r.s32() != blk[3]:
        raise Invalid("DATA block size in main header doesn't match size in DATA header")
    nch, codec = s["nch"], s["codec"]
    if blk[0] == 0x7001:
        s["kind"] = CWAV if data[:1] == b"C" else FWAV
        n = samples_to_bytes(s["sample_count"], codec)
        base = r.pos
        s["audio_offsets"] = [base + o for o in waves[:nch]]
        s["audio"] = [data[o:o + n] for o in s["audio_offsets"]]
    elif blk[0] == 0x4004:
        s["kind"] = CSTP if data[:1] == b"C" else FSTP
        regions = []
        for _ in range(r.s32()):                  # PrefetchData.ReadPrefetchData
            base = r.pos
            start, size = r.s32(), r.s32()
            r.s32()
            regions.append(dict(start_sample=start, size=size, sample_count=bytes_to_samples(cdiv(size, nch), codec),
                                audio=r.ref(base)[2]))
        first = regions[0]
        size, il = first["size"], s["interleave_size"]
        # DeInterleave(Size, InterleaveSize, ChannelCount, Size): sequential reads, every output Size bytes long
        insz = size // nch
        inb = -(-insz // il)
        last = insz - (inb - 1) * il
        outs = [bytearray(size) for _ in range(nch)]
        pos = first["audio"]
        for b in range(inb):
            cur = last if b == inb - 1 else il
            for o in range(nch):
                outs[o][il * b:il * b + cur] = data[pos:pos + cur]
                pos += cur
        # Common.ToAudioStream: the first region, not looping
        s.update(regions=regions, stream_looping=s["looping"], stream_sample_count=s["sample_count"], looping=False,
                 sample_count=first["sample_count"])
        n = samples_to_bytes(s["sample_count"], codec)
        s["audio_full"] = [bytes(o) for o in outs]
        s["audio"] = [bytes(o[:n]) for o in outs]
    else:
        raise Invalid("a stream")
    return s


def read_image(data):
    data = bytes(data)
    return _read_rwav(data) if data[:1] == b"R" else _read_bcf(data)


# ---------------------------------------------------------------- seeded random files
WAVE_VERSIONS = {CWAV: [0x02000000, 0x02010000, 0x02010100, 0x02010200], FWAV: [0x00010000, 0x00010100, 0x00010200, 0x00010300]}
STREAM_VERSIONS = {CSTP: [0x02000000, 0x02010000, 0x02030000], FSTP: [0x00020000, 0x00030000, 0x00040000, 0x00050000]}


def random_file(rng, gc_payload, kind=None, codec=None, nch=None, n=None, big=None, gaps=None):
    """rng: numpy Generator.  gc_payload(n, hist1, hist2) -> (adpcm bytes, coefs16) from the CPU oracle.
    -> (image, what the builder was given)"""
    kind = int(rng.integers(0, 5)) if kind is None else kind
    codec = int(rng.integers(0, 3)) if codec is None else codec
    nch = int(rng.integers(1, 9)) if nch is None else nch
    n = int(rng.integers(0, 3000)) if n is None else n
    big = (kind == RWAV or bool(rng.integers(0, 2))) if big is None else big
    rate = int(rng.integers(8000, 48001))
    looping = bool(rng.integers(0, 2)) and n > 0
    loop_start = int(rng.integers(0, n + 1)) if looping else 0
    audio, infos = [], []
    for _ in range(nch):
        if codec == GCADPCM:
            h1, h2 = (int(v) for v in rng.integers(-3000, 3000, 2))
            adpcm, coefs = gc_payload(n, h1, h2)
            audio.append(bytes(adpcm))
            infos.append(([int(v) for v in coefs], int(rng.integers(0, 100)), [adpcm[0] if len(adpcm) else 0, h1, h2],
                          [int(v) for v in rng.integers(-3000, 3000, 3)]))
        else:
            audio.append(rng.integers(0, 256, samples_to_bytes(n, codec), dtype="uint8").tobytes())
            infos.append(([0] * 16, 0, [0] * 3, [0] * 3))
    given = dict(kind=kind, big=big, codec=codec, nch=nch, sample_rate=rate, looping=looping, loop_start=loop_start,
                 sample_count=n, audio=audio, infos=infos)
    order = [int(v) for v in rng.permutation(nch)]
    gaps = [int(v) for v in rng.integers(0, 16, nch)] if gaps is None else gaps
    filler = rng.integers(0, 256, 64, dtype="uint8").tobytes()
    if kind == RWAV:
        given["version"] = 0x01020000
        return build_rwav(codec, rate, n, audio, infos, looping, loop_start, (1, 2), order, gaps, filler, int(rng.integers(0, 9))), given
    if kind in (CWAV, FWAV):
        version = WAVE_VERSIONS[kind][int(rng.integers(0, 4))]
        given.update(version=version, loop_start_unaligned=int(rng.integers(0, 1000)))
        return build_bcfwav(kind, big, version, codec, rate, n, audio, infos, looping, loop_start, given["loop_start_unaligned"],
                            order, gaps, filler, int(rng.integers(0, 9))), given
    versions = STREAM_VERSIONS[kind]
    version = versions[int(rng.integers(0, len(versions)))]
    il = int(rng.integers(1, 5)) * (8 if codec == GCADPCM else 2) * int(rng.integers(1, 40))
    regions = [(int(rng.integers(0, 1000)), audio)]
    for _ in range(int(rng.integers(0, 3))):      # later regions: present in the file, not read
        regions.append((int(rng.integers(0, 1000)), [rng.integers(0, 256, int(rng.integers(0, 64)), dtype="uint8").tobytes()] * nch))
    given.update(version=version, interleave_size=il, looping=False, stream_looping=looping, regions=len(regions),
                 start_sample=regions[0][0], sample_count=bytes_to_samples(len(audio[0]), codec))
    given["audio"] = [a[:samples_to_bytes(given["sample_count"], codec)] for a in audio]
    return build_prefetch(kind, big, version, codec, rate, regions, il, infos, nch, looping, loop_start, max(n, 1) * 7,
                          gaps[0], filler), given
