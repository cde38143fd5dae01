"""world_size-2 gloo test of the N>1 path on CPU: contiguous channel sharding, no data-path
collective, the final gather of every rank's bitstream and coefficients to rank 0 (BitstreamGather,
SURVEY.md 8e), max-over-ranks timing.  Each rank's
"device work" is stood in for by the oracle (checker) so the gathered result can be compared
with a single-process run over all channels."""
import os
import subprocess
import sys
import textwrap

import numpy as np

from vgaudio_amd.distributed import shard_channels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_channels_partition():
    for total in (0, 1, 7, 8, 4096, 32768, 4097):
        for world in (1, 2, 3, 8):
            blocks = [shard_channels(total, world, r) for r in range(world)]
            assert sum(c for _, c in blocks) == total
            pos = 0
            for first, count in blocks:
                assert first == pos and count in (total // world, total // world + 1)
                pos += count
    assert shard_channels(32768, 8, 3) == (3 * 4096, 4096)      # BASELINE configs[4]: 4096 per GPU


WORKER = textwrap.dedent("""
    import os, sys, time
    sys.path.insert(0, {root!r})
    import numpy as np, torch, torch.distributed as dist
    from vgaudio_amd import distributed as vd, synth
    from oracle import pyoracle as po
    rank, local_rank, world = vd.env_world()
    vd.init("gloo")
    total, n = {total}, 14 * 200 + 3
    first, count = vd.shard_channels(total, world, rank)
    counts = [vd.shard_channels(total, world, r)[1] for r in range(world)]
    pcm = synth.generate(count, n, first_channel=first)           # each rank generates only its shard
    t0 = time.perf_counter()
    coefs, adpcm = po.gc_encode_batch(pcm, threads=1)
    dt = time.perf_counter() - t0
    allc = vd.gather_channel_metadata(torch.from_numpy(coefs), counts)
    tmax = vd.max_over_ranks(dt, torch.device("cpu"))
    assert tmax >= dt
    np.save(os.path.join({out!r}, f"adpcm_{{rank}}.npy"), adpcm)
    # SURVEY.md 8e: the final gather of the BITSTREAM (and coefficients) to rank 0, in channel chunks
    pitch = (adpcm.shape[1] + 15) // 16 * 16
    rows = torch.zeros((count, pitch), dtype=torch.uint8)
    rows[:, :adpcm.shape[1]] = torch.from_numpy(np.ascontiguousarray(adpcm))
    g = vd.BitstreamGather(counts, pitch, torch.device("cpu"), chunk_channels=2)
    g.gather(rows, torch.from_numpy(coefs).reshape(count, 16))
    works = g.gather(rows, torch.from_numpy(coefs).reshape(count, 16), async_op=True, nbytes=adpcm.shape[1])      # and the asynchronous form, with digests
    for w in works:
        w.wait()
    if rank == 0:
        np.save(os.path.join({out!r}, "coefs_all.npy"), allc.numpy())
        np.save(os.path.join({out!r}, "gathered_adpcm.npy"), g.all_adpcm[:, :adpcm.shape[1]].numpy())
        np.save(os.path.join({out!r}, "gathered_coefs.npy"), g.all_coefs.numpy())
        assert g.verify(rows, torch.from_numpy(coefs).reshape(count, 16), adpcm.shape[1]).startswith("own rows identical")
        # a peer's rows arriving permuted, or stale by one byte, must not pass
        keep = g.all_adpcm.clone()
        f1 = g.firsts[1]
        g.all_adpcm[[f1, f1 + 1]] = g.all_adpcm[[f1 + 1, f1]]
        assert "wrong digest: [1]" in g.verify(rows, torch.from_numpy(coefs).reshape(count, 16), adpcm.shape[1])
        g.all_adpcm.copy_(keep)
        g.all_adpcm[f1 + 2, 5] ^= 1
        assert "wrong digest: [1]" in g.verify(rows, torch.from_numpy(coefs).reshape(count, 16), adpcm.shape[1])
        g.all_adpcm.copy_(keep)
        assert g.verify(rows, torch.from_numpy(coefs).reshape(count, 16), adpcm.shape[1]).startswith("own rows identical")
    # the barrier as a collective on a CPU tensor: dist.barrier() probes for an accelerator, which opens the GPU in every
    # rank, and these ranks stand in for GPUs on the CPU
    dist.all_reduce(torch.zeros(1))
    dist.destroy_process_group()
""")


def test_two_rank_gloo_sharded_encode(tmp_path):
    """the ranks are started by the launcher `python bench.py --gpus N` uses (distributed.launch_local_ranks)"""
    from vgaudio_amd.distributed import launch_local_ranks
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=str(tmp_path), total=7))
    assert launch_local_ranks([str(script)], 2, timeout=240) == 0
    from oracle import pyoracle as po
    from vgaudio_amd import synth
    pcm = synth.generate(7, 14 * 200 + 3)
    coefs, adpcm = po.gc_encode_batch(pcm)
    got = np.load(tmp_path / "coefs_all.npy")
    assert (got == coefs).all()
    parts = np.concatenate([np.load(tmp_path / f"adpcm_{r}.npy") for r in range(2)])
    assert (parts == adpcm).all()
    # the gathered bitstream on rank 0 is the single-process result, channel for channel
    assert (np.load(tmp_path / "gathered_adpcm.npy") == adpcm).all()
    assert (np.load(tmp_path / "gathered_coefs.npy").reshape(7, 16) == np.asarray(coefs).reshape(7, 16)).all()


def test_eight_rank_gloo_sharded_encode_uneven_counts(tmp_path):
    """BASELINE configs[4]'s world size: eight ranks, 35 channels (shares of 5 and 4), every rank's rows and coefficients
    gathered to rank 0 in channel order with the digests verified for all eight"""
    from vgaudio_amd.distributed import launch_local_ranks, shard_channels
    script = tmp_path / "worker8.py"
    script.write_text(WORKER.format(root=ROOT, out=str(tmp_path), total=35))
    assert launch_local_ranks([str(script)], 8, timeout=400) == 0
    counts = [shard_channels(35, 8, r)[1] for r in range(8)]
    assert sorted(set(counts)) == [4, 5] and sum(counts) == 35
    from oracle import pyoracle as po
    from vgaudio_amd import synth
    pcm = synth.generate(35, 14 * 200 + 3)
    coefs, adpcm = po.gc_encode_batch(pcm, threads=4)
    assert (np.load(tmp_path / "coefs_all.npy") == coefs).all()
    parts = [np.load(tmp_path / f"adpcm_{r}.npy") for r in range(8)]
    assert [p.shape[0] for p in parts] == counts
    assert (np.concatenate(parts) == adpcm).all()
    assert (np.load(tmp_path / "gathered_adpcm.npy") == adpcm).all()
    assert (np.load(tmp_path / "gathered_coefs.npy").reshape(35, 16) == np.asarray(coefs).reshape(35, 16)).all()


def test_launcher_reports_a_failing_rank_and_stops_the_others(tmp_path):
    from vgaudio_amd.distributed import launch_local_ranks
    script = tmp_path / "fail.py"
    script.write_text("import os, sys, time\n"
                      "assert os.environ['WORLD_SIZE'] == '3' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
                      "if os.environ['RANK'] == '1':\n    sys.exit(7)\n"
                      "time.sleep(60)\n")
    import time
    t0 = time.monotonic()
    assert launch_local_ranks([str(script)], 3, timeout=120) == 7
    assert time.monotonic() - t0 < 30


def test_launcher_retries_a_taken_rendezvous_port_and_nothing_else(tmp_path):
    """A deterministic failure of rank 0 is final at the first attempt (round 4's advisor: it used to be run three times
    when it happened within 15 s); a rendezvous port somebody else holds gives rank 0 the exit code the launcher retries on."""
    import socket
    import time
    from vgaudio_amd.distributed import RENDEZVOUS_PORT_TAKEN, launch_local_ranks
    marker = tmp_path / "attempts"
    script = tmp_path / "fail0.py"
    script.write_text("import os, sys\n"
                      "if os.environ['RANK'] == '0':\n"
                      "    open(%r, 'a').write('x')\n    sys.exit(9)\n"
                      "import time; time.sleep(30)\n" % str(marker))
    t0 = time.monotonic()
    assert launch_local_ranks([str(script)], 2, timeout=60) == 9
    assert marker.read_text() == "x" and time.monotonic() - t0 < 20          # one attempt
    busy = socket.socket()
    busy.bind(("127.0.0.1", 0))
    busy.listen(1)
    try:
        script2 = tmp_path / "init.py"
        script2.write_text("import sys\nsys.path.insert(0, %r)\nfrom vgaudio_amd import distributed as d\nd.init('gloo', timeout_s=20)\n" % ROOT)
        assert launch_local_ranks([str(script2)], 2, master_port=busy.getsockname()[1], timeout=90) == RENDEZVOUS_PORT_TAKEN
    finally:
        busy.close()


def test_job_description_lists_every_rank(tmp_path):
    """bench.py's N > 1 line carries what the backend itself reports: world size, one entry per rank (gathered with the job's
    own collective), the backend's name -- the first run on real multi-GPU hardware must be checkable from its line alone"""
    import json
    from vgaudio_amd.distributed import launch_local_ranks
    script = tmp_path / "job.py"
    script.write_text("import json, os, sys\nsys.path.insert(0, %r)\nimport torch\nfrom vgaudio_amd import distributed as d\n"
                      "d.init('gloo', timeout_s=60)\njob = d.describe_job(torch.device('cpu'))\n"
                      "if os.environ['RANK'] == '0':\n    json.dump(job, open(%r, 'w'))\n" % (ROOT, str(tmp_path / "job.json")))
    assert launch_local_ranks([str(script)], 3, timeout=120) == 0
    job = json.load(open(tmp_path / "job.json"))
    assert job["backend"] == "gloo" and job["world_size_reported_by_backend"] == 3 and job["world_size_env"] == 3
    assert sorted(r["rank"] for r in job["ranks"]) == [0, 1, 2] and len({r["pid"] for r in job["ranks"]}) == 3
    assert job["rccl_version"] is None and job["shared_devices"] is False


def test_launcher_passes_rank_zero_stdout_through(tmp_path):
    script = tmp_path / "echo.py"
    script.write_text("import os\nprint('line from rank', os.environ['RANK'], os.environ['LOCAL_RANK'], flush=True)\n")
    code = ("import sys; sys.path.insert(0, %r); from vgaudio_amd.distributed import launch_local_ranks; "
            "sys.exit(launch_local_ranks([%r], 2, timeout=60))" % (ROOT, str(script)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    assert r.stdout.strip() == "line from rank 0 0"           # one line on stdout: rank 0's
    assert "line from rank 1 1" in r.stderr


def test_bench_result_line_survives_failing_and_hanging_multi_gpu_extras():
    """bench.py's N > 1 extras run under `guarded`: an exception is named in the line, a hang ends with the line printed"""
    import json
    sys.path.insert(0, ROOT)
    import bench
    assert bench.guarded(None, {"metric": "m"}, lambda: (1, 2)) == (1, 2)
    res = bench.guarded(None, {"metric": "m"}, lambda: 1 // 0)
    assert "ZeroDivisionError" in res["error"]
    code = ("import sys, time; sys.path.insert(0, %r); import bench; "
            "bench.guarded(None, {'metric': 'm', 'value': 1.0}, lambda: time.sleep(60), limit_s=0.5)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "m" and line["value"] == 1.0 and "did not finish" in line["gather"]["error"]
