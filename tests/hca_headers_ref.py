"""HCA headers the encoder never writes, and frames to go with them (test code only).

Every header the encoder makes has TrackCount 1, resolutions 1..15, no ATH curve, the channel config
SetChannelConfiguration picks and one of the band layouts CriHcaEncoder.cs:288-368 derives.  Files can carry a dec chunk,
an ath chunk, a version below 0x200, any track count and channel config, any band split and up to 8 HFR groups.  This
module builds such headers (as file images through container_readers_ref, and as the HcaInfo HcaReader.cs:100-210 derives
from them) and three kinds of frames for them: encoder frames re-read under another header, structured frames (pyref
channel state filled at random and packed with pyref.pack_frame) and random bits behind a sync word."""
import math

import numpy as np

import container_readers_ref as ref
from oracle import pyoracle as po
from oracle.pyref import crihca as pyref

FIELDS = [n for n, _ in po.HcaInfo._fields_]


def _ceil_div(v, d):
    """Extensions.DivideByRoundUp: (int)Math.Ceiling((double)v / d)"""
    return int(math.ceil(v / d))


def _i16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


class Header:
    """One file header.  comp = (frame_size, tracks, config, total, base, stereo, per_hfr);
    dec = (frame_size, tracks, config, total_minus1, base_minus1, stereo_type); ath = None (no chunk) or its value."""

    def __init__(self, name, nch, comp=None, dec=None, rate=48000, version=0x0200, ath=None, frame_count=3, inserted=128,
                 appended=64, direct=False):
        self.name, self.nch, self.comp, self.dec, self.rate = name, nch, comp, dec, rate
        self.direct = direct               # an HcaInfo handed to the decoder as is: frame sizes up to 65535, no file
        self.version, self.ath, self.frame_count, self.inserted, self.appended = version, ath, frame_count, inserted, appended

    def __repr__(self):
        return self.name

    def chunks(self):
        out = [ref.hca_fmt(self.nch, self.rate, self.frame_count, self.inserted, self.appended)]
        if self.comp is not None:
            fs, tracks, config, total, base, stereo, per_hfr = self.comp
            out.append(ref.hca_comp(_i16(fs), 1, 15, tracks, config, total, base, stereo, per_hfr))
        if self.dec is not None:
            fs, tracks, config, total_m1, base_m1, stereo_type = self.dec
            out.append(ref.hca_dec(_i16(fs), 1, 15, total_m1, base_m1, tracks, config, stereo_type))
        if self.ath is not None:
            out.append(ref.hca_ath(self.ath))
        out.append(ref.hca_pad())
        return out

    def image(self, frames):
        return ref.hca_image(self.chunks(), bytes(frames), version=self.version)

    def expected(self):
        """The HcaInfo HcaReader.ReadHcaHeader (:59-121, chunk readers :140-202) and CalculateHfrValues derive."""
        h = dict.fromkeys(FIELDS, 0)
        h.update(channel_count=self.nch, sample_rate=self.rate, frame_count=self.frame_count, inserted_samples=self.inserted,
                 appended_samples=self.appended, sample_count=self.frame_count * 1024 - self.inserted - self.appended)
        h["header_size"] = len(self.image(b""))
        if self.comp is not None:
            fs, tracks, config, total, base, stereo, per_hfr = self.comp
            h.update(frame_size=fs if self.direct else _i16(fs), min_resolution=1, max_resolution=15, track_count=tracks, channel_config=config,
                     total_band_count=total, base_band_count=base, stereo_band_count=stereo, bands_per_hfr_group=per_hfr)
        if self.dec is not None:
            fs, tracks, config, total_m1, base_m1, stereo_type = self.dec
            h.update(frame_size=_i16(fs), min_resolution=1, max_resolution=15, total_band_count=total_m1 + 1,
                     base_band_count=base_m1 + 1, track_count=tracks, channel_config=config)
            if stereo_type == 0:
                h["base_band_count"] = h["total_band_count"]
            else:
                h["stereo_band_count"] = h["total_band_count"] - h["base_band_count"]
        if self.ath is not None:
            h["use_ath_curve"] = int(self.ath == 1)
        elif self.version < 0x0200:
            h["use_ath_curve"] = 1
        h["track_count"] = max(h["track_count"], 1)
        if h["bands_per_hfr_group"] > 0:
            h["hfr_band_count"] = h["total_band_count"] - h["base_band_count"] - h["stereo_band_count"]
            h["hfr_group_count"] = _ceil_div(h["hfr_band_count"], h["bands_per_hfr_group"])
        return h

    def info(self):
        info = po.HcaInfo()
        for k, v in self.expected().items():
            setattr(info, k, v)
        return info

    def pyref_info(self):
        h = pyref.HcaInfo()
        for k, v in self.expected().items():
            setattr(h, k, v)
        h.use_ath_curve = bool(h.use_ath_curve)
        return h


def comp(name, nch, fs=0x200, tracks=1, config=0, total=100, base=60, stereo=20, per_hfr=5, **kw):
    return Header(name, nch, comp=(fs, tracks, config, total, base, stereo, per_hfr), **kw)


def dec(name, nch, fs=0x200, tracks=1, config=0, total=100, base=60, stereo_type=1, **kw):
    return Header(name, nch, dec=(fs, tracks, config, total - 1, base - 1, stereo_type), **kw)


def families():
    """{family: [Header]}: the header space the encoder leaves out"""
    F = {}
    F["ath"] = ([comp(f"ath_v103_{r}", 2, rate=r, version=0x0103) for r in (8000, 22050, 44100, 48000, 96000, 0xFFFFFF)]
                + [comp(f"ath_chunk1_{r}", 1, rate=r, ath=1, stereo=0) for r in (8000, 44100, 0xFFFFFF)]
                + [comp("ath_chunk0_v103", 2, version=0x0103, ath=0), comp("ath_chunk1_v200", 2, ath=1)])
    F["tracks"] = [comp(f"tracks{t}_ch{c}", c, tracks=t, config=0, stereo=20 if s else 0)
                   for c in range(1, 9) for t in range(1, 9) for s in (0, 1) if (c + t) % 3 == 0 or t <= 2]
    F["config"] = [comp(f"config{k}_ch{c}", c, config=k, fs=0x300) for c in (4, 5) for k in range(16)]
    F["bands"] = [comp(f"bands_t{t}_b{b}_s{s}_h{h}", 2, total=t, base=b, stereo=s, per_hfr=h, fs=0x300)
                  for (t, b, s) in ((128, 20, 0), (128, 64, 0), (128, 40, 24), (100, 60, 20), (90, 80, 10), (128, 120, 8),
                                    (60, 50, 20), (40, 30, 0), (128, 1, 0), (16, 2, 3))
                  for h in (0, 1, 3, 7, 16) if h == 0 or _ceil_div(t - b - s, h) <= 8]
    F["dec"] = [dec(f"dec_t{t}_b{b}_st{st}_ch{c}", c, total=t, base=b, stereo_type=st, fs=0x300)
                for (t, b) in ((100, 60), (50, 60), (60, 60), (128, 128), (10, 128), (1, 1), (128, 129), (256, 60),
                               (256, 256), (50, 200))
                for st in (0, 2) for c in (1, 2)]
    F["frame_size"] = [comp(f"fs{fs}_ch{c}", c, fs=fs, total=t, base=b, stereo=s, per_hfr=h, frame_count=fc)
                       for fs, fc in ((8, 4), (9, 4), (255, 3), (4097, 2))
                       for (c, t, b, s, h) in ((1, 128, 128, 0, 0), (2, 100, 60, 20, 5), (3, 128, 96, 32, 0), (8, 64, 24, 8, 4))]
    return F


# ---------------------------------------------------------------- frames
def _valid_q(rng, res):
    if res == 0:
        return 0
    if res < 8:
        return int(rng.integers(-res, res + 1))
    m = (1 << (pyref.Tables.get().quantized_spectrum_max_bits[res] - 1)) - 1
    return int(rng.integers(-m, m + 1))


def _fill(frame, rng, intensity_max, spectra):
    frame.acceptable_noise_level = int(rng.integers(0, 48))
    frame.evaluation_boundary = int(rng.integers(0, 128))
    for ch in frame.channels:
        bits = int(rng.integers(0, 7))
        ch.scale_factor_delta_bits = bits
        sf = [0] * pyref.SUB
        if bits:
            sf[0] = int(rng.integers(0, 64))
            md = max((1 << (bits - 1)) - 1, 0)
            for i in range(1, min(ch.coded, pyref.SUB)):
                d = int(rng.integers(-md, md + 1)) if bits < 6 and rng.random() < 0.9 else int(rng.integers(-63, 64))
                sf[i] = min(max(sf[i - 1] + d, 0), 63)
        ch.scale_factors = sf
        for i in range(min(ch.coded, pyref.SUB)):
            noise = frame.ath_curve[i] + frame.acceptable_noise_level - (1 if i < frame.evaluation_boundary else 0)
            ch.resolution[i] = pyref.calculate_resolution(sf[i], noise)
        for s in range(pyref.SUBFRAMES):
            for i in range(min(ch.coded, pyref.SUB)):
                ch.quantized_spectra[s][i] = _valid_q(rng, ch.resolution[i]) if spectra else 0
        ch.intensity = [int(rng.integers(0, intensity_max + 1)) for _ in range(pyref.SUBFRAMES)]
        ch.hfr_scales = [int(rng.integers(0, 64)) for _ in range(8)]


def structured_frame(header, rng, intensity_max=14):
    """pyref channel state at random (scale factors with valid deltas, resolutions as the decoder derives them, in-range
    codes, intensities, HFR scales, noise level, evaluation boundary), packed.  Falls back to fewer bits when the frame
    is too small: no spectra, then no scale factors, then a bare sync word."""
    h = header.pyref_info()
    fs = h.frame_size
    try:
        frame = pyref.Frame(h)
    except IndexError:                                     # the reference throws before any frame: any bits will do
        return raw_frame(header, rng, intensity_max)
    for spectra, sfs in ((True, True), (False, True), (False, False)):
        _fill(frame, rng, intensity_max, spectra)
        if not sfs:
            for ch in frame.channels:
                ch.scale_factor_delta_bits = 0
                ch.scale_factors = [0] * pyref.SUB
                ch.resolution = [0] * pyref.SUB
        try:
            return np.frombuffer(pyref.pack_frame(frame), np.uint8)
        except (ValueError, IndexError):                   # too small a frame; more than 128 coded bands
            continue
    out = np.zeros(fs, np.uint8)
    out[:2] = 0xFF
    return out


def raw_frame(header, rng, intensity_max=15):
    """random bits behind a sync word; raw 6-bit scale factors (delta bits 6 / 7) so that delta decoding cannot fail
    (the library refuses such frames, CriHcaPacking.cs:84), intensities up to intensity_max"""
    e = header.expected()
    fs = e["frame_size"]
    bits = rng.integers(0, 2, fs * 8).astype(np.uint8)
    bits[:16] = 1
    types = channel_types(e)
    pos = 32
    for c in range(e["channel_count"]):
        coded = e["base_band_count"] if types[c] == pyref.STEREO_SECONDARY else e["base_band_count"] + e["stereo_band_count"]
        if pos + 3 > len(bits):
            break
        bits[pos:pos + 3] = (1, 1, int(rng.integers(0, 2)))
        pos += 3 + 6 * max(coded, 0)
        if types[c] == pyref.STEREO_SECONDARY:
            for _ in range(8):
                v = int(rng.integers(0, intensity_max + 1))
                for k in range(4):
                    if pos + k < len(bits):
                        bits[pos + k] = (v >> (3 - k)) & 1
                pos += 4
        elif e["hfr_group_count"] > 0:
            pos += 6 * e["hfr_group_count"]
    return np.packbits(bits)


def channel_types(e):
    """GetChannelTypes (CriHcaFrame.cs:34-52), padded with Discrete to 8 for the generator's own bookkeeping"""
    h = pyref.HcaInfo()
    for k, v in e.items():
        setattr(h, k, v)
    t = pyref.channel_types(h)
    return list(t) + [pyref.DISCRETE] * (8 - len(t))


def frames_for(header, rng, kind, intensity_max=14):
    """[frame_count, frame_size] uint8 frames of one kind: 'structured', 'raw' or 'mixed' (alternating)"""
    e = header.expected()
    out = np.zeros((e["frame_count"], e["frame_size"]), np.uint8)
    for k in range(e["frame_count"]):
        use_raw = kind == "raw" or (kind == "mixed" and k % 2 == 1)
        out[k] = raw_frame(header, rng, intensity_max) if use_raw else structured_frame(header, rng, intensity_max)
    return out


def encoder_frames(nch, n, quality="High", seed=0):
    """(info, frames [frame_count, frame_size]) from the oracle's encoder"""
    from vgaudio_amd import synth
    pcm = synth.generate(nch, n, first_channel=seed)
    rc, info, frames = po.hca_encode(pcm, po.hca_params(nch, n, quality=quality))
    assert rc == 0
    return info, np.asarray(frames, np.uint8).reshape(info.frame_count, info.frame_size)


def reference_decode(header_or_info, frames, max_frames=None):
    """pyref's CriHcaDecoder.Decode over the first max_frames frames: ('ok', pcm [nch, n]) or ('IndexError', frame)"""
    if isinstance(header_or_info, Header):
        h = header_or_info.pyref_info()
    else:
        h = pyref.HcaInfo()
        for k in FIELDS:
            setattr(h, k, getattr(header_or_info, k))
        h.use_ath_curve = bool(h.use_ath_curve)
    count = h.frame_count if max_frames is None else min(max_frames, h.frame_count)
    try:
        frame = pyref.Frame(h)
    except IndexError:
        return "IndexError", -1
    out = np.zeros((h.channel_count, count * 1024), np.int16)
    for i in range(count):
        try:
            block = pyref.decode_frame(bytes(frames[i]), frame)
        except IndexError:
            return "IndexError", i
        out[:, i * 1024:(i + 1) * 1024] = np.asarray(block, np.int16)
    return "ok", out


def oracle_frames(info, frames):
    """the C oracle's decode with every frame's raw 1024 samples kept (inserted = 0, appended = 0 over the same frames):
    (rc, pcm [nch, frame_count * 1024]); rc -6 = IndexOutOfRangeException, the PCM of the frames before it kept"""
    raw = po.HcaInfo()
    for k in FIELDS:
        setattr(raw, k, getattr(info, k))
    raw.inserted_samples = raw.appended_samples = 0
    raw.sample_count = raw.frame_count * 1024
    return po.hca_decode(raw, np.ascontiguousarray(frames).reshape(-1))
