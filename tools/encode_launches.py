#!/usr/bin/env python3
"""One process of an A/B comparison of the GC-ADPCM encoder (profiles/rNN_encode_ab.log): synthesis, coefficient search,
2 warm-up encode launches and 25 timed ones at BASELINE configs[1], the output's checksum.  Meant to run under
`rocprofv3 --kernel-trace --stats` (the kernel's own time is read from the trace, tools/trace_last_launches.py) or
`rocprofv3 --pmc`; honours VGAUDIO_HIP_LIBRARY (tools/variants/).
    python tools/encode_launches.py [channels] [launches]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vgaudio_amd import device as vdev

nch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 25
n = 2880000
d = torch.device("cuda:0")
pcm = vdev.synth_pcm(nch, n, d)
coefs = vdev.gc_coefs(pcm, n)
out = vdev.alloc_adpcm(nch, n, d)
for _ in range(2):
    vdev.gc_encode(pcm, n, coefs, out=out)
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(launches):
    vdev.gc_encode(pcm, n, coefs, out=out)
b.record()
torch.cuda.synchronize()
h = int(out.view(torch.int64).sum().item()) if out.numel() % 8 == 0 else int(out.to(torch.int64).sum().item())
print("channels %d  launches %d  encode ms per launch (events) %.3f  checksum %d" % (nch, launches, a.elapsed_time(b) / launches, h), flush=True)
