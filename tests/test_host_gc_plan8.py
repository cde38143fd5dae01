"""The queue of the GC-ADPCM encoder's self-served shape (vgaudio_amd/csrc/gc_plan8.hpp: groups of eight channel slots,
item counts, the item decode the kernel shares with the host) walked by a stand-alone program, tests/host/gc_plan8_driver.cpp,
built with AddressSanitizer and UBSan and run as a child process: 1 to 40 channels, the lengths at the edges of the
eight-frame tile, uniform and ragged, one, four and 160 pieces and a two-size schedule -- every (channel, frame) belongs to
exactly one item, and the queue is as long as the launch says.  Needs no GPU."""
import os
import platform
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_plan8_driver.cpp")
FLAGS = ["-std=c++17", "-Wall", "-fwrapv", "-ffp-contract=off", "-fno-fast-math"]


def test_every_channel_frame_belongs_to_exactly_one_item(tmp_path):
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "gc_plan8_driver")
    subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([setarch, platform.machine(), "-R", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    walked = int(r.stdout.split()[1])
    assert walked >= 3 * 40 * (11 * 3 + 3 * 4), walked


def test_the_self_served_schedule_covers_its_longest_channel_and_fills_whole_rounds():
    """the piece schedule planned for the self-served shape (the plan hook with the layout hook at 1): the pieces cover the
    longest channel whatever the batch, and at the benchmark's shape -- 4096 channels x 205 715 frames on 256 compute units --
    the big items are whole rounds of the 3072 workgroups (one piece index more at the most) and the small ones one round"""
    import ctypes as C

    import numpy as np

    from vgaudio_amd import _lib
    L = _lib.lib()

    def plan(cus, groups, frames, group_frames, ragged):
        out = (C.c_int * 5)()
        assert L.vga_testing_gc_plan_pieces(cus, groups, frames, group_frames, int(ragged), out) == 0
        return dict(pieces=out[0], big=out[1], nb=out[2], small=out[3], persistent=out[4])

    def first(p, k):
        return min(k, p["nb"]) * p["big"] + max(k - p["nb"], 0) * p["small"]

    old = L.vga_testing_gc_encoder_layout_this_thread(1)
    try:
        rng = np.random.default_rng(20261020)
        shapes = [(256, 256, 205715), (256, 128, 205715), (256, 1, 14), (256, 1, 1), (304, 19, 10 ** 7), (64, 3, 2 ** 27)]
        for _ in range(1500):
            shapes.append((int(rng.choice([8, 64, 104, 256, 304])), int(rng.integers(1, 3000)), max(int(np.exp(rng.uniform(0, np.log(2 ** 27)))), 1)))
        for ragged in (False, True):
            for cus, groups, frames in shapes:
                gf = frames * groups if not ragged else max(frames, int(frames * groups * rng.uniform(0.02, 1.0)))
                p = plan(cus, groups, frames, gf, ragged)
                assert p["persistent"] == 1 and 1 <= p["pieces"] <= 1024, p
                assert first(p, p["pieces"]) >= frames, (p, frames)
                if p["pieces"] > 1:
                    assert first(p, p["pieces"] - 1) < frames, (p, frames)
        p = plan(256, 256, 205715, 256 * 205715, False)
        wgs, groups8 = 256 * 12, 512
        # (the big pieces are equal and cover what the small ones leave: rounding can add one piece index, 512 items)
        assert (p["nb"] * groups8) % wgs <= groups8 and (p["pieces"] - p["nb"]) * groups8 == wgs, p
    finally:
        L.vga_testing_gc_encoder_layout_this_thread(old)
