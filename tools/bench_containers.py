#!/usr/bin/env python3
"""Measurements for the SURVEY 8f rows (containers, WAVE transposes, encryption passes): device-resident kernel
times and the HBM traffic they stand for (bytes read + written / time).  Prints one JSON object.

    python tools/bench_containers.py          (--pcm: the copy ceiling and the PCM stream rows only)

The bank read of wave and prefetch files (vga_nwwav_bank_read_device against one copy per channel) is timed by
tools/bench_nwwav_bank.py, which prints its own JSON line.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return min(a.elapsed_time(b) for a, b in evs)


def pcm_rows(L, dev, st, rec, n):
    """BFSTM PCM16 / PCM8 images (vgaudio_hip_pcm.h): 4096 channels x 60 s as 2048 stereo files, written from and read
    to int16 rows (PCM16 big-endian: a byte swap each way; PCM8: EncodeSigned / DecodeSigned), device-resident"""
    import torch
    from vgaudio_amd import _lib
    nf, nch = 2048, 2
    pitch = (n + 15) // 16 * 16
    rows = torch.randint(-32768, 32768, (nf * nch, pitch), dtype=torch.int16, device=dev)
    for codec, name in ((1, "pcm16"), (0, "pcm8")):
        p = _lib.NwParamsC()
        p.target, p.sample_rate, p.sample_count, p.endianness = 2, 48000, n, -1
        lay = _lib.NwLayoutC()
        _lib.check(L.vga_nwstm_pcm_layout_for(C.byref(p), codec, nch, C.byref(lay)))
        fpitch = (lay.file_size + 255) // 256 * 256
        files = torch.empty((nf, fpitch), dtype=torch.uint8, device=dev)
        ms = timed(lambda: _lib.check(L.vga_nwstm_pcm_write_device(C.byref(p), codec, nch, nf, None, rows.data_ptr(), 0, pitch,
                                                                   files.data_ptr(), fpitch, st())))
        rec("nwstm_%s_write" % name, ms, nf * nch * n * 2 + nf * lay.file_size, channels=nf * nch, files=nf,
            note="BFSTM %s from int16 rows: header + converting interleave, every image byte written once" % name.upper())
        info = _lib.NwInfoC()
        one = files[0, :lay.file_size].cpu().numpy()
        _lib.check(L.vga_nwstm_pcm_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(info)))
        back = torch.empty_like(rows)
        ms = timed(lambda: _lib.check(L.vga_nwstm_pcm_read_device(C.byref(info), files.data_ptr(), fpitch, nf, back.data_ptr(), 0,
                                                                  pitch, st())))
        if codec == 1:
            assert torch.equal(back[:, :n], rows[:, :n])
        else:
            assert torch.equal(back[:, :n], (rows[:, :n] >> 8) << 8)
        rec("nwstm_%s_read" % name, ms, nf * nch * info.adpcm_bytes + nf * nch * n * 2, channels=nf * nch, files=nf,
            note="BFSTM %s DATA -> int16 rows" % name.upper())
        del files, back
    del rows


def main():
    import torch
    from vgaudio_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = lambda: torch.cuda.current_stream().cuda_stream
    out = {}

    def rec(name, ms, nbytes, **kw):
        out[name] = dict(ms=round(ms, 3), GB_per_s=round(nbytes / ms / 1e6, 1), bytes_moved=int(nbytes), **kw)

    # what a plain device copy reaches on this box (read + write), for scale
    src = torch.empty(1 << 32, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src))
    rec("hbm_copy_ceiling", ms, 2 * src.numel(), note="torch copy_ of 4 GiB")
    del src, dst
    if "--pcm" in sys.argv[1:]:                             # the ceiling and the PCM stream rows only
        pcm_rows(L, dev, st, rec, 60 * 48000)
        print(json.dumps(out))
        return

    n = 60 * 48000
    # DSP image: 1024 channels x 60 s of GC-ADPCM (1.69 GB image)
    nch = 1024
    nb = L.vga_gcadpcm_sample_count_to_byte_count(n)
    pitch = (nb + 15) // 16 * 16
    adpcm = torch.randint(0, 256, (nch, pitch), dtype=torch.uint8, device=dev)
    coefs = torch.zeros((nch, 16), dtype=torch.int16, device=dev)
    p = _lib.DspParamsC(48000, n, 0, 0, 0, 0x3800, 1, 1)
    lay = _lib.DspLayoutC()
    _lib.check(L.vga_dsp_layout_for(C.byref(p), nch, C.byref(lay)))
    image = torch.empty(lay.file_size, dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_dsp_write_device(adpcm.data_ptr(), pitch, nb, coefs.data_ptr(), None, None, None, nch,
                                                         C.byref(p), image.data_ptr(), st())))
    rec("dsp_image", ms, nch * nb + 2 * lay.file_size, channels=nch, note="memset + header + interleave (read once, image written twice)")
    del adpcm, image

    # ADX image: 255 channels x 60 s (413 MB image), 18-byte frames -> 2-byte granules
    nch = 255
    ap = _lib.AdxParams()
    L.vga_adx_default_params(C.byref(ap))
    anb = L.vga_adx_encoded_byte_count(n, C.byref(ap))
    apitch = (anb + 15) // 16 * 16
    audio = torch.randint(0, 256, (nch, apitch), dtype=torch.uint8, device=dev)
    hist = torch.zeros(nch, dtype=torch.int16, device=dev)
    fp = _lib.AdxFileParamsC(48000, n, 0, 0, 0, 0, 18, 4, 3, 500, 0, 1)
    al = _lib.AdxFileLayoutC()
    _lib.check(L.vga_adx_file_layout_for(C.byref(fp), nch, C.byref(al)))
    image = torch.empty(al.file_size, dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_adx_write_device(audio.data_ptr(), apitch, anb, hist.data_ptr(), nch, C.byref(fp),
                                                         image.data_ptr(), st())))
    rec("adx_image", ms, nch * anb + 2 * al.file_size, channels=nch)
    del image

    # ADX encryption pass in place, config-3 shape (4096 channels)
    nch = 4096
    audio = torch.randint(0, 256, (nch, apitch), dtype=torch.uint8, device=dev)
    key = _lib.AdxKeyC()
    L.vga_adx_key_from_string(b"karaage", C.byref(key))
    ms = timed(lambda: _lib.check(L.vga_adx_crypt_device(audio.data_ptr(), apitch, anb, nch, C.byref(key), 8, 18, st())))
    rec("adx_crypt", ms, nch * anb, channels=nch, note="reads every frame (emptiness test), writes 2 of 18 bytes")
    del audio

    # WAVE transposes: 64 channels x 60 s (369 MB of samples)
    nch = 64
    inter = torch.randint(0, 256, (n * nch * 2,), dtype=torch.uint8, device=dev)
    ppitch = (n + 7) // 8 * 8
    planar = torch.empty((nch, ppitch), dtype=torch.int16, device=dev)
    ms = timed(lambda: _lib.check(L.vga_wave_deinterleave_pcm16_device(inter.data_ptr(), n, nch, planar.data_ptr(), ppitch, st())))
    rec("wave_deinterleave", ms, 4 * n * nch, channels=nch)
    wp = _lib.WaveParamsC(48000, n, 0, 0, 0)
    size = L.vga_wave_file_size(C.byref(wp), nch)
    wfile = torch.empty(size, dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_wave_write_pcm16_device(planar.data_ptr(), ppitch, nch, C.byref(wp), wfile.data_ptr(), st())))
    rec("wave_write", ms, 4 * n * nch, channels=nch, note="includes a synchronous 136-byte header upload")
    del inter, planar, wfile

    # HCA encryption pass, config-4 shape (1024 stereo streams, 2813 frames of 682 bytes)
    ns, fc, fs = 1024, 2813, 682
    fpitch = (fc * fs + 15) // 16 * 16
    frames = torch.randint(0, 256, (ns, fpitch), dtype=torch.uint8, device=dev)
    import numpy as np
    dec, enc = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    _lib.check(L.vga_hca_key_tables(56, 0xCC55463930DBE1AB, dec.ctypes.data_as(_lib.u8p), enc.ctypes.data_as(_lib.u8p)))
    ms = timed(lambda: _lib.check(L.vga_hca_crypt_device(frames.data_ptr(), fpitch, ns, fc, fs, enc.ctypes.data_as(_lib.u8p), st())))
    rec("hca_crypt", ms, 2 * ns * fc * fs, streams=ns, note="includes the 256-byte table upload and a stream sync")
    info = _lib.HcaInfoC()
    hp = _lib.HcaParamsC(2, 0, 0, 2, 48000, n, 0, 0, 0)
    _lib.check(L.vga_hca_encoder_initialize(C.byref(hp), C.byref(info)))
    fsz = L.vga_hca_file_size(C.byref(info))
    files = torch.empty((ns, fsz + 14), dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_hca_write_device(C.byref(info), frames.data_ptr(), fpitch, ns, None, 1.0, 0, 0,
                                                         files.data_ptr(), fsz + 14, st())))
    rec("hca_images", ms, 2 * ns * info.frame_count * info.frame_size, streams=ns)

    # BFSTM images: 4096 channels x 60 s as 2048 stereo files, one launch per kernel for the whole batch
    nf, nch = 2048, 2
    nwp = _lib.NwParamsC()
    nwp.target, nwp.sample_rate, nwp.sample_count, nwp.endianness = 2, 48000, n, -1
    nwl = _lib.NwLayoutC()
    _lib.check(L.vga_nwstm_layout_for(C.byref(nwp), nch, C.byref(nwl)))
    nb = nwl.channel_adpcm_bytes
    pitch = (nb + 15) // 16 * 16
    adpcm = torch.randint(0, 256, (nf * nch, pitch), dtype=torch.uint8, device=dev)
    coefs = torch.zeros((nf * nch, 16), dtype=torch.int16, device=dev)
    ne = nwl.channel_seek_entries
    seek = torch.zeros((nf * nch, 2 * ne), dtype=torch.int16, device=dev)
    fpitch = (nwl.file_size + 255) // 256 * 256
    files = torch.empty((nf, fpitch), dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_nwstm_write_device(C.byref(nwp), nch, nf, None, adpcm.data_ptr(), pitch, nb,
                                                           coefs.data_ptr(), None, None, None, seek.data_ptr(), 2 * ne, ne,
                                                           files.data_ptr(), fpitch, st())))
    rec("nwstm_write", ms, nf * nch * nb + nf * nwl.file_size, channels=nf * nch, files=nf,
        note="BFSTM: header + seek + interleave kernels, every image byte written once")
    info = _lib.NwInfoC()
    one = files[0, :nwl.file_size].cpu().numpy()
    _lib.check(L.vga_nwstm_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(info)))
    back = torch.empty_like(adpcm)
    ms = timed(lambda: _lib.check(L.vga_nwstm_read_device(C.byref(info), files.data_ptr(), fpitch, nf, back.data_ptr(), pitch,
                                                          st())))
    assert torch.equal(back[:, :nb], adpcm[:, :nb])
    rec("nwstm_read", ms, 2 * nf * nch * info.adpcm_bytes, channels=nf * nch, files=nf, note="BFSTM DATA -> pitched channels")
    del adpcm, seek, files, back
    pcm_rows(L, dev, st, rec, n)

    # the file readers: one image built on the host, replicated over the batch (the kernels do not look at the bytes)
    def tile(img, count):
        fp = (len(img) + 255) // 256 * 256
        t = torch.zeros((count, fp), dtype=torch.uint8, device=dev)
        t[:, :len(img)] = torch.from_numpy(img).to(dev)
        return t, fp

    rng = np.random.default_rng(1)
    # DSP: 2048 stereo files of 60 s
    nf, nch = 2048, 2
    dp = _lib.DspParamsC(48000, n, 0, 0, 0, 0x3800, 1, 1)
    dl = _lib.DspLayoutC()
    _lib.check(L.vga_dsp_layout_for(C.byref(dp), nch, C.byref(dl)))
    nb = L.vga_gcadpcm_sample_count_to_byte_count(n)
    rows = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(nch)]
    img = np.zeros(dl.file_size, np.uint8)
    co = np.zeros((nch, 16), np.int16)
    _lib.check(L.vga_dsp_write((_lib.u8p * nch)(*[r.ctypes.data_as(_lib.u8p) for r in rows]), nb, co.ctypes.data_as(_lib.i16p), None,
                               None, None, nch, C.byref(dp), img.ctypes.data_as(_lib.u8p)))
    di = _lib.DspInfoC()
    _lib.check(L.vga_dsp_parse(img.ctypes.data_as(_lib.u8p), len(img), C.byref(di)))
    files, fp = tile(img, nf)
    pitch = (nb + 15) // 16 * 16
    back = torch.empty((nf * nch, pitch), dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_dsp_read_device(C.byref(di), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st())))
    assert all(torch.equal(back[c::nch, :nb], torch.from_numpy(rows[c]).to(dev).expand(nf, nb)) for c in range(nch))
    rec("dsp_read", ms, 2 * nf * nch * nb, channels=nf * nch, files=nf, note="DSP audio -> pitched channels (interleave 8 KiB)")
    del files, back

    # HPS, IDSP and GENH: 2048 stereo files of 60 s, device-resident
    adpcm = torch.randint(0, 256, (nf * nch, pitch), dtype=torch.uint8, device=dev)
    coefs = torch.zeros((nf * nch, 16), dtype=torch.int16, device=dev)
    back = torch.empty_like(adpcm)
    hp = _lib.HpsParamsC(48000, n, 0, 0, 0)
    hl = _lib.HpsLayoutC()
    _lib.check(L.vga_hps_layout_for(C.byref(hp), nch, C.byref(hl)))
    fp = (hl.file_size + 255) // 256 * 256
    files = torch.empty((nf, fp), dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_hps_write_device(C.byref(hp), nch, nf, adpcm.data_ptr(), pitch, nb, coefs.data_ptr(), None, None,
                                                         None, 0, 0, files.data_ptr(), fp, st())))
    rec("hps_write", ms, nf * nch * nb + nf * hl.file_size, channels=nf * nch, files=nf, blocks_per_file=hl.block_count,
        note="header kernel (stream + block headers) + body kernel, every image byte written once")
    hi = _lib.HpsInfoC()
    one = files[0, :hl.file_size].cpu().numpy()
    _lib.check(L.vga_hps_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(hi), None, 0))
    hb = (_lib.HpsBlockInfoC * hi.block_count)()
    _lib.check(L.vga_hps_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(hi), hb, hi.block_count))
    ms = timed(lambda: _lib.check(L.vga_hps_read_device(C.byref(hi), hb, files.data_ptr(), fp, nf, back.data_ptr(), pitch, st())))
    assert torch.equal(back[:, :nb], adpcm[:, :nb])
    rec("hps_read", ms, 2 * nf * nch * nb, channels=nf * nch, files=nf, note="block gather -> pitched channels")
    del files
    ip = _lib.IdspParamsC(48000, n, 0, 0, 0, 0x10, 1)
    il = _lib.IdspLayoutC()
    _lib.check(L.vga_idsp_layout_for(C.byref(ip), nch, C.byref(il)))
    fp = (il.file_size + 255) // 256 * 256
    files = torch.empty((nf, fp), dtype=torch.uint8, device=dev)
    ms = timed(lambda: _lib.check(L.vga_idsp_write_device(C.byref(ip), nch, nf, adpcm.data_ptr(), pitch, nb, coefs.data_ptr(), None, None,
                                                          None, files.data_ptr(), fp, st())))
    rec("idsp_write", ms, nf * nch * nb + nf * il.file_size, channels=nf * nch, files=nf,
        note="header kernel + batched interleave (BlockSize 0x10), every image byte written once")
    ii = _lib.IdspInfoC()
    one = files[0, :il.file_size].cpu().numpy()
    _lib.check(L.vga_idsp_parse(one.ctypes.data_as(_lib.u8p), len(one), C.byref(ii)))
    back.zero_()
    ms = timed(lambda: _lib.check(L.vga_idsp_read_device(C.byref(ii), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st())))
    assert torch.equal(back[:, :nb], adpcm[:, :nb])
    rec("idsp_read", ms, 2 * nf * nch * nb, channels=nf * nch, files=nf, note="de-interleave of 16-byte blocks")
    del files
    # GENH: the IDSP images' audio region read as GENH (interleave 0x10), the header in front of it
    import struct
    hdr = np.zeros(il.header_size, np.uint8)
    struct.pack_into("<4s14i", hdr, 0, b"GENH", nch, 0x10, 48000, -1, n, 12, il.header_size, 0x40, 0x40, 0x40, 0, 0, 0, 0)
    gi = _lib.GenhInfoC()
    probe = np.concatenate([hdr, np.zeros(nch * nb, np.uint8)])
    _lib.check(L.vga_genh_parse(probe.ctypes.data_as(_lib.u8p), len(probe), C.byref(gi)))
    files = torch.empty((nf, fp), dtype=torch.uint8, device=dev)
    _lib.check(L.vga_idsp_write_device(C.byref(ip), nch, nf, adpcm.data_ptr(), pitch, nb, coefs.data_ptr(), None, None, None,
                                       files.data_ptr(), fp, st()))
    back.zero_()
    ms = timed(lambda: _lib.check(L.vga_genh_read_device(C.byref(gi), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st())))
    assert torch.equal(back[:, :nb - 16], adpcm[:, :nb - 16])   # GENH's short last block sits differently from IDSP's padded one
    rec("genh_read", ms, 2 * nf * nch * nb, channels=nf * nch, files=nf,
        note="de-interleave of 16-byte blocks, an unpadded 3-byte last block (GENH header)")
    del files, back, adpcm

    # ADX: 2048 stereo files of 60 s, 18-byte frames; the 16-byte-vector kernel and the general de-interleave
    ap = _lib.AdxFileParamsC(48000, n, 0, 0, 0, 0, 18, 4, 3, 500, 0, 1)
    al = _lib.AdxFileLayoutC()
    _lib.check(L.vga_adx_file_layout_for(C.byref(ap), nch, C.byref(al)))
    ab = al.frame_count * 18
    rows = [rng.integers(0, 256, ab, dtype=np.uint8) for _ in range(nch)]
    img = np.zeros(al.file_size, np.uint8)
    hist = np.zeros(nch, np.int16)
    _lib.check(L.vga_adx_write((_lib.u8p * nch)(*[r.ctypes.data_as(_lib.u8p) for r in rows]), ab, hist.ctypes.data_as(_lib.i16p), nch,
                               C.byref(ap), img.ctypes.data_as(_lib.u8p)))
    ai = _lib.AdxFileInfoC()
    _lib.check(L.vga_adx_parse(img.ctypes.data_as(_lib.u8p), len(img), C.byref(ai)))
    files, fp = tile(img, nf)
    pitch = (ab + 15) // 16 * 16
    back = torch.empty((nf * nch, pitch), dtype=torch.uint8, device=dev)
    read = lambda: _lib.check(L.vga_adx_read_device(C.byref(ai), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st()))
    ms = timed(read)
    assert all(torch.equal(back[c::nch, :ab], torch.from_numpy(rows[c]).to(dev).expand(nf, ab)) for c in range(nch))
    L.vga_testing_adx_read_general_this_thread(1)
    ms_general = timed(read)
    L.vga_testing_adx_read_general_this_thread(0)
    assert all(torch.equal(back[c::nch, :ab], torch.from_numpy(rows[c]).to(dev).expand(nf, ab)) for c in range(nch))
    rec("adx_read", ms, 2 * nf * nch * ab, channels=nf * nch, files=nf, general_path_ms=round(ms_general, 3),
        general_path_GB_per_s=round(2 * nf * nch * ab / ms_general / 1e6, 1),
        note="18-byte frames: 16-byte vectors through LDS; general_path = the 2-byte-granule de-interleave")
    del files, back

    # HCA: 1024 stereo streams of 60 s, quality High, every frame's CRC-16 checked
    ns = 1024
    info = _lib.HcaInfoC()
    hp = _lib.HcaParamsC(2, 0, 0, 2, 48000, n, 0, 0, 0)
    _lib.check(L.vga_hca_encoder_initialize(C.byref(hp), C.byref(info)))
    fb = info.frame_count * info.frame_size
    fr = rng.integers(0, 256, fb, dtype=np.uint8)
    img = np.zeros(L.vga_hca_file_size(C.byref(info)), np.uint8)
    _lib.check(L.vga_hca_write(C.byref(info), fr.ctypes.data_as(_lib.u8p), None, 1.0, 0, 0, img.ctypes.data_as(_lib.u8p)))
    hi = _lib.HcaFileInfoC()
    _lib.check(L.vga_hca_parse(img.ctypes.data_as(_lib.u8p), len(img), C.byref(hi)))
    files, fp = tile(img, ns)
    pitch = (fb + 8 + 15) // 16 * 16
    back = torch.empty((ns, pitch), dtype=torch.uint8, device=dev)
    bad = torch.empty(ns, dtype=torch.int32, device=dev)
    ms = timed(lambda: _lib.check(L.vga_hca_read_device(C.byref(hi), files.data_ptr(), fp, ns, back.data_ptr(), pitch, bad.data_ptr(),
                                                        st())))
    assert torch.equal(back[:, :fb], torch.from_numpy(fr).to(dev).expand(ns, fb))
    rec("hca_read", ms, 2 * ns * fb, streams=ns, frames_per_stream=info.frame_count, frame_size=info.frame_size,
        note="frames copied to the decoder's layout, CRC-16 of every frame checked (random frames: all counted bad)")
    del files, back
    print(json.dumps(out))


if __name__ == "__main__":
    main()
