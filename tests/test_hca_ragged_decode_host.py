"""vga_hca_decode_batch_v sorts its streams into shape classes before it buckets them by length (vgaudio_amd/csrc/capi_hca_v.hip):
two streams share their launches exactly when the kernels' view of them -- the DeviceInfo that make_device_info() builds --
agrees once frame_count, sample_count and inserted_samples are ignored.  vga_testing_hca_decode_classes returns those classes;
host code, no GPU.  The infos come from vga_hca_encoder_initialize (CriHcaEncoder.cs:61-114), which needs none either."""
import ctypes as C
import time

import numpy as np

from vgaudio_amd import _lib

QUALITY = dict(Highest=1, High=2, Middle=3, Low=4, Lowest=5)
DEVICE_INFO_BYTES = 240
PER_STREAM = ("frame_count", "sample_count", "inserted_samples")


def info(nch=2, n=48000, rate=48000, quality="High", loop=None):
    cp = _lib.HcaParamsC(QUALITY[quality], 0, 0, nch, rate, n, 0, 0, 0)
    if loop:
        cp.looping, cp.loop_start, cp.loop_end = 1, loop[0], loop[1]
    h = _lib.HcaInfoC()
    _lib.check(_lib.lib().vga_hca_encoder_initialize(C.byref(cp), C.byref(h)))
    return h


def classes(infos):
    arr = (_lib.HcaInfoC * max(len(infos), 1))(*infos)
    out = (C.c_int * max(len(infos), 1))()
    n = _lib.lib().vga_testing_hca_decode_classes(arr, len(infos), out)
    return n, list(out[:len(infos)])


def test_streams_that_differ_in_length_only_share_a_class():
    infos = [info(n=n) for n in (1, 1000, 1024, 48000, 48001, 2_880_000)]
    assert len({h.frame_count for h in infos}) > 3
    n, cls = classes(infos)
    assert n == 1 and cls == [0] * len(infos)


def test_a_looping_and_a_plain_stream_of_one_quality_and_rate_share_a_class():
    plain, looping = info(n=50_000), info(n=50_000, loop=(3000, 40_000))
    assert looping.looping and plain.inserted_samples != looping.inserted_samples
    n, cls = classes([plain, looping])
    assert n == 1 and cls == [0, 0]


def test_fields_the_decoder_never_reads_do_not_split_a_class():
    a = info(n=30_000)
    b = _lib.HcaInfoC.from_buffer_copy(a)
    b.comment_length, b.header_size, b.appended_samples = 17, a.header_size + 32, a.appended_samples + 5
    b.looping, b.loop_start_frame, b.loop_end_frame, b.pre_loop_samples, b.post_loop_samples = 1, 2, 9, 100, 200
    assert classes([a, b]) == (1, [0, 0])


def test_quality_channel_count_and_sample_rate_split_classes():
    base = info()
    for other in (info(quality="Middle"), info(quality="Highest"), info(nch=1), info(nch=6)):
        assert classes([base, other]) == (2, [0, 1])
    # The sample rate reaches the kernels through the ATH curve alone (CriHcaFrame.ScaleAthCurve, :60-83): streams that use the
    # curve split by rate ...
    ath = [_lib.HcaInfoC.from_buffer_copy(info(rate=r)) for r in (48000, 44100, 32000)]
    for h in ath:
        h.use_ath_curve = 1
    assert classes(ath) == (3, [0, 1, 2])
    assert classes([base, ath[0]]) == (2, [0, 1])
    # ... and streams that do not (every stream the encoder writes) have one frame size, band layout and DeviceInfo per
    # quality whatever their rate -- the bitrate is a fixed fraction of the PCM's (CriHcaEncoder.cs:288-368) -- so by the rule
    # (equality of the DeviceInfo) they share a class, and their launches
    for r in (44100, 32000):
        assert _blob_with_per_stream_fields_equal(info(rate=r)) == _blob_with_per_stream_fields_equal(base)
        assert classes([base, info(rate=r)]) == (1, [0, 0])


def test_class_ids_are_dense_and_in_order_of_first_appearance():
    a, b, c = info(quality="High"), info(quality="Low"), info(nch=1)
    order = [b, b, a, c, a, b, c, info(quality="Low", n=77)]
    assert classes(order) == (3, [0, 0, 1, 2, 1, 0, 2, 0])


def test_twenty_thousand_streams_are_classified_quickly():
    """A pairwise comparison of 20 000 structs (2e8 memcmp) is what the call used to do; a hash per stream is not."""
    rng = np.random.default_rng(9)
    shapes = [info(nch=c, quality=q) for c in (1, 2, 4) for q in ("Highest", "High", "Middle", "Low")]
    infos = []
    for i in range(20_000):
        h = _lib.HcaInfoC.from_buffer_copy(shapes[int(rng.integers(0, len(shapes)))])
        h.sample_count = int(rng.integers(1, 3_000_000))              # all different lengths
        h.frame_count = (h.sample_count + h.inserted_samples + 1023) // 1024
        infos.append(h)
    arr = (_lib.HcaInfoC * len(infos))(*infos)
    out = (C.c_int * len(infos))()
    t0 = time.perf_counter()
    n = _lib.lib().vga_testing_hca_decode_classes(arr, len(infos), out)
    dt = time.perf_counter() - t0
    assert n == len(shapes) and max(out) == n - 1
    assert dt < 0.5, dt


def test_bad_arguments_are_negative():
    L = _lib.lib()
    one = (_lib.HcaInfoC * 1)(info())
    out = (C.c_int * 1)()
    assert L.vga_testing_hca_decode_classes(None, 1, out) < 0
    assert L.vga_testing_hca_decode_classes(one, 1, None) < 0
    assert L.vga_testing_hca_decode_classes(one, -1, out) < 0
    assert L.vga_testing_hca_decode_classes(None, 0, None) == 0
    bad = (_lib.HcaInfoC * 1)(info())
    bad[0].channel_count = 9                                          # an HcaInfo the decoder refuses
    assert L.vga_testing_hca_decode_classes(bad, 1, out) < 0
    stats = (C.c_longlong * 8)()
    assert L.vga_testing_hca_decode_v_stats(stats, 8) == 5 and L.vga_testing_hca_decode_v_stats(None, 0) == 5


def _blob_with_per_stream_fields_equal(h):
    g = _lib.HcaInfoC.from_buffer_copy(h)
    for f in PER_STREAM:
        setattr(g, f, 1)
    out = (C.c_uint8 * DEVICE_INFO_BYTES)()
    _lib.check(_lib.lib().vga_testing_hca_device_info(C.byref(g), out, DEVICE_INFO_BYTES))
    return bytes(out)


def test_classes_are_the_rule_as_stated():
    """two streams share a class exactly when their DeviceInfo blobs agree once the three per-stream fields are made equal"""
    rng = np.random.default_rng(3)
    infos = []
    for _ in range(120):
        n = int(rng.integers(1, 400_000))
        loop = None
        if rng.random() < 0.3 and n > 10:
            a = int(rng.integers(0, n - 1))
            loop = (a, int(rng.integers(a + 1, n + 1)))
        h = info(nch=int(rng.choice([1, 2, 2, 3, 4, 6, 8])), n=n, rate=int(rng.choice([48000, 44100, 22050])),
                 quality=str(rng.choice(list(QUALITY))), loop=loop)
        if rng.random() < 0.2:
            h.use_ath_curve = 1
        infos.append(h)
    n, cls = classes(infos)
    blobs = [_blob_with_per_stream_fields_equal(h) for h in infos]
    assert n == len(set(blobs)) > 10
    for i in range(len(infos)):
        for j in range(i):
            assert (cls[i] == cls[j]) == (blobs[i] == blobs[j]), (i, j)
