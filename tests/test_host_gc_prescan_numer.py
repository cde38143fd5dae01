"""The tile head's pre-scan word in the numerator domain (vgaudio_amd/csrc/gc_encode_core.hpp: prescan_numer_word, N1 and
N3-N7) against the reference's form -- prescan_range(x, c0, c1, 2, 14, ...) and clamp16i -- word for word, by a stand-alone
program, tests/host/gc_prescan_numer_driver.cpp, built with AddressSanitizer and UBSan and run as a child process: 10^6
seeded random frames with |c0| + |c1| <= 30720, frames at the rails, coefficient sums of exactly 30720 at every sign
combination, frames built so that D is 0, +-1, +-2047, +-2048, +-2049 at the maximising and at the minimising sample, all-zero
frames, and frames whose distances leave 16 bits either way.  Needs no GPU."""
import os
import platform
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_prescan_numer_driver.cpp")
FLAGS = ["-std=c++17", "-Wall", "-fwrapv", "-ffp-contract=off", "-fno-fast-math"]


def test_the_numerator_form_gives_the_reference_pre_scan_word(tmp_path):
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "gc_prescan_numer_driver")
    subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [SRC, "-o", exe],
                   check=True)
    r = subprocess.run([setarch, platform.machine(), "-R", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    compared, pinned = (int(v) for v in r.stdout.split()[1:3])
    assert compared >= 1000000 + 20000 + 20000 and pinned >= 1000, (compared, pinned)
