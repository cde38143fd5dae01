"""The HCA encoder kernels on the ways a frame rarely goes (tests/hca_encoder_path_cases.py): raw 6-bit scale factors, the loop
that drops bands and searches the noise level again, the intensity index at its bound of 13 and at 0, the HFR group scale by
1 / average, both exits of the boundary search, "Bitrate is set too low.".  test_hca_encoder_paths_host.py proves on the
oracle's counters that every case takes its path; here the frames of every entry point must be the oracle's byte for byte,
and the decoder's PCM of those frames the oracle's.

Both encoder kernels run every case they can take.  launch_encode (hca_encode_kernel.hip) gives one- and two-channel streams
to the wave-per-frame kernel (hca_encode_wave_kernel.hip) and everything else to the workgroup-per-run kernel;
vga_testing_hca_frames_per_group_this_thread(1000) sends the calling thread's launches to the workgroup kernel whatever
the channel count.  The library has no query for the kernel a launch took, so FORMS records the rule: form "default" is the
wave kernel for cases of one or two channels (every frame size here fits its LDS budget) and the workgroup kernel above;
form "workgroup" is the hook, run for the one- and two-channel cases only (for the others it would repeat "default")."""
import contextlib
import functools

import numpy as np
import pytest

import hca_encoder_path_cases as pc
from oracle import pyoracle as po
from test_gpu_hca import _feed
from test_gpu_hca_ragged_device import JUNK, batch_of, torch
from vgaudio_amd import _lib, crihca
from vgaudio_amd.crihca import CriHcaDecoder, CriHcaEncoder, CriHcaFormat, CriHcaParameters
from vgaudio_amd.gcadpcm import Pcm16Format

pytestmark = pytest.mark.gpu
Q = {"Highest": 1, "High": 2, "Middle": 3, "Low": 4, "Lowest": 5}
BY_NAME = {c.name: c for c in pc.CASES + pc.ERROR_CASES}
CHANNELS = {c.name: c.make().shape[0] for c in pc.CASES + pc.ERROR_CASES}


def forms_of(name):
    return ["default", "workgroup"] if CHANNELS[name] <= 2 else ["default"]


def kernel_of(name, form):
    return "wave" if form == "default" and CHANNELS[name] <= 2 else "workgroup"


FORMS = [(c.name, f) for c in pc.CASES for f in forms_of(c.name)]
ERROR_FORMS = [(c.name, f) for c in pc.ERROR_CASES for f in forms_of(c.name)]
# the raw-scale-factor, repeated-drop, intensity-13 and inverse-HFR cases (and the looping one) for the entry points besides the
# batch call
OTHER_ENTRY_CASES = ["raw_impulse4_mono_highest", "raw_impulse4_mono_highest_looping", "drops_impulse4_mono_high",
                     "intensity13_left_silent_lowest", "hfr_inverse_alternating_stereo_low", "drops_noise_3ch_lowest_24000",
                     "raw_second_pair_of_4_middle"]
OTHER_FORMS = [(n, f) for n in OTHER_ENTRY_CASES for f in forms_of(n)]


@contextlib.contextmanager
def form(which):
    old = _lib.lib().vga_testing_hca_frames_per_group_this_thread(1000 if which == "workgroup" else 0)
    try:
        yield
    finally:
        _lib.lib().vga_testing_hca_frames_per_group_this_thread(old)


def test_the_forms_cover_both_kernels():
    assert {kernel_of(n, f) for n, f in FORMS} == {"wave", "workgroup"}
    for path in pc.PATHS:
        claiming = [c.name for c in pc.CASES + pc.ERROR_CASES if path in c.paths]
        assert {kernel_of(n, f) for n in claiming for f in forms_of(n)} == {"wave", "workgroup"}, path


class Ref:
    """one stream under a case's parameters: PCM, and the oracle's return code, HcaInfo, frames and decode of them"""

    def __init__(self, case, x):
        self.case, self.pcm = case, x
        self.params = pc.oracle_params(case, x)
        self.rc, self.oinfo, frames = po.hca_encode(x, self.params)
        self.frames2d = frames
        self.frames = frames.reshape(-1)
        self.info = _lib.HcaInfoC()
        for f, _ in po.HcaInfo._fields_:
            setattr(self.info, f, getattr(self.oinfo, f))
        if self.rc == 0:
            rc, want = po.hca_decode(self.oinfo, frames)
            assert rc == 0
            self.want = np.ascontiguousarray(want)

    def pcm16(self):
        p = Pcm16Format(list(self.pcm), self.case.rate)
        if self.case.loop:
            p.Looping, p.LoopStart, p.LoopEnd = True, self.case.loop[0], self.case.loop[1]
        return p

    def config(self, **kw):
        return CriHcaParameters(Quality=Q[self.case.quality], Bitrate=self.case.bitrate, LimitBitrate=self.case.limit, **kw)


@functools.lru_cache(maxsize=None)
def trio(name):
    """the case's stream between two ordinary synthetic streams of its shape and parameters"""
    case = BY_NAME[name]
    x = case.make()
    nch, n = x.shape
    return [Ref(case, pc.ordinary(nch, n, first_channel=16)), Ref(case, x), Ref(case, pc.ordinary(nch, n, first_channel=40))]


@functools.lru_cache(maxsize=None)
def ragged_set(name):
    """the case's stream among ordinary (for "too low" cases: silent) streams of its parameters and other lengths"""
    case = BY_NAME[name]
    x = case.make()
    nch = x.shape[0]
    other = (lambda n, k: np.zeros((nch, n), np.int16)) if name.startswith("too_low_after_silent") else \
        (lambda n, k: pc.ordinary(nch, n, first_channel=8 * k))
    lengths = (9500, 9000, 11000, 9001) if case.loop else (3000, 0, 7777, 1)          # (a loop end lies inside its stream)
    return [Ref(case, other(lengths[0], 1)), Ref(case, other(lengths[1], 2)), Ref(case, x), Ref(case, other(lengths[2], 3)),
            Ref(case, other(lengths[3], 4))]


def same_info(got, want, what):
    for k, v in want.as_dict().items():
        assert getattr(got, k) == v, (what, k, getattr(got, k), v)


def same_frames(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(np.asarray(got) != want)
    assert bad.size == 0, (what, "first difference at [frame, byte]", bad[0].tolist(), "of", len(bad))


# ---------------------------------------------------------------- the batch call, every case, both kernels
@pytest.mark.parametrize("name,which", FORMS)
def test_encode_matches_oracle(name, which):
    """CriHcaFormat.EncodeBatchFromPcm16 of [ordinary, the case, ordinary]: HcaInfo and frames of all three are the oracle's --
    the case's rare path must not leak into its neighbours, whose launches it shares"""
    refs = trio(name)
    assert all(r.rc == 0 for r in refs)
    with form(which):
        fmts = CriHcaFormat.EncodeBatchFromPcm16([r.pcm16() for r in refs], refs[1].config())
    for k, (r, fmt) in enumerate(zip(refs, fmts)):
        same_info(fmt.Hca.c, r.oinfo, (name, which, k))
        same_frames(fmt.AudioData, r.frames2d, (name, kernel_of(name, which), "stream", k))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_decode_matches_oracle(name):
    """CriHcaDecoder.Decode of the ORACLE's frames (raw scale factors, intensity 13 and 0, the inverse HFR scale and frames
    without their highest bands as a real encoder writes them) is the oracle's PCM, for all three streams of the batch"""
    refs = trio(name)
    dec = CriHcaDecoder.Decode(crihca.HcaInfo(refs[1].info), [r.frames2d for r in refs])
    for k, (r, d) in enumerate(zip(refs, dec)):
        got = np.stack(d)
        assert got.shape == r.want.shape, (name, k)
        bad = np.argwhere(got != r.want)
        assert bad.size == 0, (name, "stream", k, "first difference at [channel, sample]", bad[0].tolist(), "of", len(bad))


# ---------------------------------------------------------------- the other entry points
@pytest.mark.parametrize("name,which", OTHER_FORMS)
def test_streaming_encoder_matches_oracle(name, which):
    """CriHcaEncoder.Encode / GetPendingFrame, 1024 samples at a time"""
    r = trio(name)[1]
    nch, n = r.pcm.shape
    loop = r.case.loop
    cfg = r.config(ChannelCount=nch, SampleRate=r.case.rate, SampleCount=n, Looping=bool(loop), LoopStart=loop[0] if loop else 0,
                   LoopEnd=loop[1] if loop else 0)
    with form(which):
        enc = CriHcaEncoder.InitializeNew(cfg)
        try:
            same_info(enc.Hca.c, r.oinfo, (name, which))
            got, _ = _feed(enc, r.pcm, n, nch, enc.FrameSize, garbage_tail=False)
        finally:
            enc.close()
    same_frames(got, r.frames2d, (name, kernel_of(name, which)))


@pytest.mark.parametrize("name,which", OTHER_FORMS)
def test_ragged_host_call_matches_oracle(name, which):
    """crihca.encode_files (vga_hca_encode_batch_v): the case among streams of its own parameters and other lengths (where
    nothing loops, one empty and one of a single sample) and two streams of another shape"""
    refs = ragged_set(name)
    others = [Ref(BY_NAME["raw_impulse4_mono_highest"], pc.ordinary(1, 2500, first_channel=3)),
              Ref(BY_NAME["hfr_inverse_alternating_stereo_low"], pc.ordinary(2, 5000, first_channel=5))]
    files = others[:1] + refs + others[1:]
    assert all(r.rc == 0 for r in files)
    with form(which):
        fmts = crihca.encode_files([r.pcm16() for r in files], [r.config() for r in files])
    for k, (r, fmt) in enumerate(zip(files, fmts)):
        same_info(fmt.Hca.c, r.oinfo, (name, which, k))
        same_frames(fmt.AudioData, r.frames2d, (name, which, "file", k))


@pytest.mark.parametrize("name,which", [(n, f) for n, f in OTHER_FORMS if not BY_NAME[n].loop])
def test_ragged_device_call_matches_oracle(name, which):
    """crihca.RaggedHca.encode_device (vga_hca_encode_device_v): packed PCM in, packed frames out, every stream's status
    word 0, nothing written outside the streams' own frames"""
    refs = ragged_set(name)
    with form(which), batch_of(refs) as b:
        pcm, frames, st = b.encode()
        torch().cuda.synchronize()
        assert np.all(st.cpu().numpy() == 0), (name, which, st.cpu().numpy().tolist())
        b.check_frames(frames.cpu().numpy(), (name, kernel_of(name, which)))
        assert np.array_equal(pcm.cpu().numpy(), b.pcm_image()), "d_pcm is an input"


# ---------------------------------------------------------------- "Bitrate is set too low."
@pytest.mark.parametrize("name,which", ERROR_FORMS)
def test_refused_stream_raises_what_the_oracle_returns(name, which):
    """the oracle's -3 is the reference's InvalidDataException("Bitrate is set too low."): the batch call and the streaming
    object raise InvalidDataError with that message, whichever frame of the stream is the first that does not fit"""
    r = trio(name)[1]
    assert r.rc == -3 == _lib.VGA_ERR_INVALID_DATA
    nch, n = r.pcm.shape
    with form(which):
        with pytest.raises(_lib.InvalidDataError, match="Bitrate is set too low"):
            CriHcaFormat().EncodeFromPcm16(r.pcm16(), r.config())
        enc = CriHcaEncoder.InitializeNew(r.config(ChannelCount=nch, SampleRate=r.case.rate, SampleCount=n))
        try:
            with pytest.raises(_lib.InvalidDataError, match="Bitrate is set too low"):
                _feed(enc, r.pcm, n, nch, enc.FrameSize, garbage_tail=False)
        finally:
            enc.close()


@pytest.mark.parametrize("name,which", [("too_low_impulse4_3ch_11250", "default"), ("too_low_after_silent_frames_stereo_8000", "default"),
                                        ("too_low_after_silent_frames_stereo_8000", "workgroup")])
def test_one_refused_stream_among_good_ones(name, which):
    """The reference converts a batch file by file and catches per file (VGAudio.Cli/Batch.cs:24-44): the file whose encoder
    throws is reported, the others are written.  The host batch calls are one call with one error, so they raise as the
    failing file's CriHcaFormat.EncodeFromPcm16 does and hand out nothing; the per-file outcome is what the device-resident
    call reports: the refused stream's status word carries the "too low" bit (4) and no other, its neighbours' words are 0
    and their frames the oracle's, and nothing outside the streams' own frames is written."""
    refs = ragged_set(name)
    assert [r.rc for r in refs] == [0, 0, -3, 0, 0]
    with form(which):
        with pytest.raises(_lib.InvalidDataError, match="Bitrate is set too low"):
            crihca.encode_files([r.pcm16() for r in refs], [r.config() for r in refs])
        if name == "too_low_impulse4_3ch_11250":                       # (its ordinary neighbours of equal length fit)
            same = trio(name)
            assert [s.rc for s in same] == [0, -3, 0]
            with pytest.raises(_lib.InvalidDataError, match="Bitrate is set too low"):
                CriHcaFormat.EncodeBatchFromPcm16([s.pcm16() for s in same], same[1].config())
        with batch_of(refs) as b:
            pcm, frames, st = b.encode()
            torch().cuda.synchronize()
            assert st.cpu().numpy()[:len(refs)].tolist() == [0, 0, 4, 0, 0], (name, which)
            got = frames.cpu().numpy()
            own = np.zeros(got.size, bool)
            for k, (r, at) in enumerate(zip(refs, b.fo)):
                own[at:at + r.frames.size] = True
                if r.rc == 0:
                    assert np.array_equal(got[at:at + r.frames.size], r.frames), (name, which, "stream", k)
            assert np.all(got[~own] == JUNK), (name, which, "wrote outside the streams' own frames")
