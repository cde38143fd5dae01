"""The case table of include/vgaudio_hip_files/hca_ragged_loops.h, shared by tests/test_hca_ragged_loops_host.py (CPU) and
tests/test_gpu_hca_ragged_loops.py: looping streams at the smallest shapes at which the packed encoder's stream map can go wrong,
interleaved with plain streams, per shape class; and what the CPU oracle says about each.  48 kHz, default quality, no stream
over 24 frames.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np

from oracle import pyoracle as po
from vgaudio_amd import _lib, crihca

# (file samples, loop start, loop end)
LOOP_CASES = [
    (20000, 3000, 15000),    # 1: one whole cleared frame in front (inserted 2248), audio behind the loop end, post 360
    (9000, 1024, 9000),      # 2: loop start on a frame boundary, loop to the end, post 256
    (5000, 0, 5000),         # 3
    (1500, 1000, 1400),      # 4: six frames, three of them cleared (inserted 4248)
    (300, 100, 300),         # 5: a short loop that ends with the file: the replay runs past the row's end in chunk 0, reads zeros
    (2950, 2900, 2950),      # 6: the same in chunk 2: the src[a - 1024] branch of fetch_pcm
    (4096, 4000, 4096),      # 7: the replay reaches a chunk beyond last_chunk
    (20000, 14640, 15000),   # 8a: loop 360 = post: the predicate's boundary, independent of the tail
    (20000, 14641, 15000),   # 8b: loop 359 < post: reads the tail
]
# parameter sets whose oracle frames DO change with the audio behind SampleCount (predicate 1)
TAIL_READERS = [(20000, 14641, 15000), (20000, 14800, 15000), (5000, 100, 300), (3000, 2900, 2950)]


def L():
    return _lib.lib()


def params_of(nch, n, loop=None):
    return po.hca_params(nch, n, looping=bool(loop), loop_start=loop[0] if loop else 0, loop_end=loop[1] if loop else 0)


def info_of(params):
    """the library's HcaInfo for the oracle's params (CriHcaEncoder.Initialize, host code)"""
    h = _lib.HcaInfoC()
    cp = _lib.HcaParamsC(*[getattr(params, f) for f, _ in po.HcaParams._fields_])
    _lib.check(L().vga_hca_encoder_initialize(C.byref(cp), C.byref(h)))
    return h


def post_and_loop(h):
    """(post audio samples, loop length) as the header's comment defines them"""
    post = h.frame_count * 1024 - h.inserted_samples - h.appended_samples - h.sample_count
    return post, h.sample_count - (h.loop_start_frame * 1024 + h.pre_loop_samples - h.inserted_samples)


def noise_behind(pcm, sample_count, seed=99):
    """a copy of [nch, n] PCM with everything behind sample_count replaced by noise"""
    out = np.array(pcm, dtype=np.int16)
    tail = out.shape[1] - sample_count
    if tail > 0:
        out[:, sample_count:] = np.random.default_rng(seed).integers(-30000, 30000, (out.shape[0], tail), dtype=np.int16)
    return out


class Stream:
    """one stream: the file's params and PCM, the oracle's frames of the WHOLE file and its decode of them"""

    def __init__(self, nch, n, k, loop=None):
        self.n, self.loop = n, loop
        self.params = params_of(nch, n, loop)
        self.pcm = po.synth_generate(nch, max(n, 1), first_channel=8 * k)[:, :n]
        rc, oi, frames = po.hca_encode(self.pcm, self.params)
        assert rc == 0, (nch, n, loop)
        self.oinfo, self.frames = oi, frames.reshape(-1)
        self.info = info_of(self.params)
        assert all(getattr(self.info, f) == getattr(oi, f) for f, _ in po.HcaInfo._fields_)
        rc, want = po.hca_decode(oi, frames)
        assert rc == 0
        self.want = np.ascontiguousarray(want)                       # [nch, sample_count]
        self.may_read_tail = crihca.loop_may_read_tail(self.info)

    @property
    def row_is_the_file(self):
        """the packed encode must equal the oracle on the whole file"""
        return not self.may_read_tail or self.n == self.info.sample_count


def samples_for(frames, rng):
    """a sample count that gives `frames` frames (a plain stream leads in with 128 samples)"""
    return frames * 1024 - 128 - int(rng.integers(0, 1024 if frames > 1 else 800))


def make_class(nch, seed):
    """the loop cases interleaved with plain streams of 1 to 24 frames, one of a single frame and one of no samples among them"""
    rng = np.random.default_rng(seed)
    plain = [500, 0, samples_for(24, rng)]
    while len(plain) < len(LOOP_CASES) + 1:
        n = samples_for(int(rng.integers(1, 25 if nch <= 2 else 10)), rng)
        if n not in plain:
            plain.append(n)
    streams = []
    for k, n in enumerate(plain):
        streams.append(Stream(nch, n, 2 * k))
        if k < len(LOOP_CASES):
            c = LOOP_CASES[k]
            streams.append(Stream(nch, c[0], 2 * k + 1, loop=c[1:]))
    assert all(1 <= s.info.frame_count <= 24 for s in streams)
    return streams


_CLASSES = {}


def classes():
    """{"mono", "stereo": the one-wave kernel's; "six": hca_encode_kernel's}, made once per process"""
    if not _CLASSES:
        _CLASSES.update({"mono": make_class(1, 20261101), "stereo": make_class(2, 20261102), "six": make_class(6, 20261106)})
    return _CLASSES
