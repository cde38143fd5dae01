"""The parameter table of tests/test_hca_initialize_host.py and tests/test_hca_host_layer.py (test code only):
CriHcaParameters over which CriHcaEncoder.Initialize (CriHcaEncoder.cs:61-114) is held to the oracle.

Seven axes; every value of every axis meets two values of every other axis, the rest at the base case.  A case is the
nine ints of vga_hca_params: (quality, bitrate, limit_bitrate, channel_count, sample_rate, sample_count, looping,
loop_start, loop_end)."""
import itertools

CHANNELS = list(range(1, 9))
QUALITIES = [0, 1, 2, 3, 4, 5]                          # NotSet, Highest .. Lowest
RATES = [8000, 22050, 32000, 44100, 48000, 96000]
COUNTS = [0, 1, 127, 128, 896, 897, 1023, 1024, 1025, 2047, 99_999]
BITRATES = [0, 1, 8000, 96000, 10_000_000]               # the last is above a quarter of any PCM rate here (at most 3 072 000)
LIMITS = [0, 1]
# None: no loop.  (loop_start, where loop_end lies): -1 below sample_count, 0 at it, +1 beyond it
LOOPS = [None] + [(start, end) for start in (0, 1, 1023, 1024, 3000) for end in (-1, 0, 1)]

AXES = [("channels", CHANNELS), ("quality", QUALITIES), ("rate", RATES), ("count", COUNTS), ("bitrate", BITRATES),
        ("limit", LIMITS), ("loop", LOOPS)]
BASE = dict(channels=2, quality=2, rate=48000, count=99_999, bitrate=0, limit=0, loop=None)
# the two values of an axis that every value of the other axes meets: where the derivation branches
PARTNERS = dict(channels=[1, 6], quality=[1, 5], rate=[22050, 96000], count=[897, 2047], bitrate=[1, 96000], limit=[0, 1],
                loop=[(1, -1), (3000, 1)])


def params_of(channels, quality, rate, count, bitrate, limit, loop):
    if loop is None:
        return (quality, bitrate, limit, channels, rate, count, 0, 0, 0)
    start, where = loop
    end = {-1: count // 2, 0: count, 1: count + 500}[where]
    return (quality, bitrate, limit, channels, rate, count, 1, start, end)


# loop padding to a 2048-byte boundary (CalculateHeaderSize :400-418), by hand: 2 ch High at 48 kHz has frames of 682 bytes
# and a header of 96: a loop that starts in frame 0 is padded by (2048 - 96) / 682 = 2 whole frames and 588 header bytes.
# 8 ch Highest at 48 kHz has frames of 4096 bytes: the padding is below one frame, bytes only.
PADDING_INSERTS_FRAMES = (2, 0, 0, 2, 48000, 99_999, 1, 0, 50_000)
PADDING_INSERTS_NONE = (1, 0, 0, 8, 48000, 99_999, 1, 0, 50_000)
# frame_size 0 (bitrate 1: 1 * 1024 / rate / 8) in a looping stream: the reference divides by FrameSize (:411)
LOOPING_FRAME_SIZE_0 = (2, 1, 0, 2, 48000, 99_999, 1, 1024, 50_000)
# refused before anything is derived
REFUSED = [(2, 0, 0, 0, 48000, 5000, 0, 0, 0), (2, 0, 0, 9, 48000, 5000, 0, 0, 0), (2, 0, 0, 2, 0, 5000, 0, 0, 0)]
# the library refuses a negative sample count; the reference and the oracle do not check it (listed in the change that
# added this table; not compared with the oracle)
NEGATIVE_COUNT = (2, 0, 0, 2, 48000, -1, 0, 0, 0)


def cases():
    seen, out = set(), []

    def add(p):
        if p not in seen:
            seen.add(p)
            out.append(p)

    for (a, values), (b, _) in itertools.permutations(AXES, 2):
        for v in values:
            for w in PARTNERS[b]:
                add(params_of(**dict(BASE, **{a: v, b: w})))
    for p in [PADDING_INSERTS_FRAMES, PADDING_INSERTS_NONE, LOOPING_FRAME_SIZE_0] + REFUSED:
        add(p)
    return out


# Where the library refuses: its code and message ON THE PARENT of the change that moved Initialize into hca_host.hpp,
# recorded from a run of that commit (the yardstick, not the moved code).  Every other case of the table succeeds there.
LOW, CHANNELS_MSG, RATE_MSG = (-3, "Bitrate is set too low."), (-2, "HCA channel count must be 8 or below"), (-1, "bad sample rate / count")
PARENT_REFUSALS = {
    (2, 1, 0, 2, 48000, 99999, 1, 0, 49999): LOW, (2, 1, 0, 2, 48000, 99999, 1, 0, 99999): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 0, 100499): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1, 49999): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 1, 99999): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1, 100499): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 1023, 49999): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1023, 99999): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 1023, 100499): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1024, 49999): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 1024, 99999): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1024, 100499): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 3000, 49999): LOW, (2, 1, 0, 2, 48000, 99999, 1, 3000, 99999): LOW,
    (2, 1, 0, 2, 48000, 99999, 1, 3000, 100499): LOW, (2, 1, 0, 2, 48000, 99999, 1, 1024, 50000): LOW,
    (2, 0, 0, 0, 48000, 5000, 0, 0, 0): CHANNELS_MSG, (2, 0, 0, 9, 48000, 5000, 0, 0, 0): CHANNELS_MSG,
    (2, 0, 0, 2, 0, 5000, 0, 0, 0): RATE_MSG,
    NEGATIVE_COUNT: RATE_MSG,
}
