// capi_gc_channels.hip -- C-ABI entry points for GC-ADPCM channel metadata (alignment re-encode, seek table, loop context)
// and the DSP container (see include/vgaudio_hip.h).  The layouts and the alignment plan are gc_host.hpp's.
#include "gc_capi.hpp"

using namespace vga;

extern "C" {

// ---------------------------------------------------------------- channel metadata
int vga_gcadpcm_channel_layout_for(const vga_gcadpcm_channel_params *p, vga_gcadpcm_channel_layout *out) { return gc::channel_layout_for(p, out); }
size_t vga_gcadpcm_build_channels_workspace_bytes(int nch, const vga_gcadpcm_channel_params *p) { return gc::build_channels_workspace_bytes(nch, p); }

int vga_gcadpcm_build_channels_device(const uint8_t *d_adpcm, int64_t adpcm_pitch, const int16_t *d_coefs, int nch,
                                      const vga_gcadpcm_channel_params *p, uint8_t *d_adpcm_out, int64_t out_pitch,
                                      int16_t *d_pcm_out, int64_t pcm_pitch, int16_t *d_seek_out, int64_t seek_pitch,
                                      int16_t *d_loop_context_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    vga_gcadpcm_channel_layout L;
    if (int rc = gc::channel_layout_for(p, &L)) return rc;
    if (nch < 0) { set_error("negative channel count"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    hipStream_t st = (hipStream_t)stream;
    const int n_al = L.sample_count_aligned;
    const int bytes_in = gc::sample_count_to_byte_count(L.alignment_needed ? p->loop_end : p->sample_count);
    const int bytes_al = gc::sample_count_to_byte_count(n_al);
    if (int rc = gc::check_adpcm_layout(d_adpcm, adpcm_pitch, bytes_in, "vga_gcadpcm_build_channels_device (input)")) return rc;
    if (L.alignment_needed && !d_adpcm_out) {
        set_error("the loop needs alignment: adpcm_out is required");
        return VGA_ERR_ARGUMENT;
    }
    if (d_adpcm_out)
        if (int rc = gc::check_adpcm_layout(d_adpcm_out, out_pitch, bytes_al, "vga_gcadpcm_build_channels_device (output)")) return rc;
    if (d_pcm_out)
        if (int rc = gc::check_pcm_layout(d_pcm_out, pcm_pitch, n_al, "vga_gcadpcm_build_channels_device (pcm)")) return rc;
    if (d_seek_out && seek_pitch < 2 * (int64_t)L.seek_table_entries) { set_error("seek table pitch too small"); return VGA_ERR_ARGUMENT; }
    if (workspace_bytes < gc::build_channels_workspace_bytes(nch, p) || !d_workspace || ((uintptr_t)d_workspace & 15)) {
        set_error("workspace too small or not 16-byte aligned: need %zu bytes", gc::build_channels_workspace_bytes(nch, p));
        return VGA_ERR_ARGUMENT;
    }
    const bool want_ctx = d_loop_context_out != nullptr;
    gc::ChannelsPlan plan;
    if (int rc = gc::plan_channels(p, L, nch, want_ctx, plan)) return rc;

    uint8_t *w = static_cast<uint8_t *>(d_workspace);
    int16_t *pcm = d_pcm_out ? d_pcm_out : reinterpret_cast<int16_t *>(w);
    const int64_t ppitch = d_pcm_out ? pcm_pitch : plan.ws_pcm_pitch;
    const bool want_seek = d_seek_out && L.seek_table_entries > 0;
    const bool ctx_needs_pcm = want_ctx && L.loop_start_aligned != 0;
    if (L.alignment_needed) {                                   // GcAdpcmAlignment.cs:33-62
        int16_t *new_pcm = reinterpret_cast<int16_t *>(w + plan.new_pcm_at);
        int16_t *h1 = reinterpret_cast<int16_t *>(w + plan.hist1_at), *h2 = reinterpret_cast<int16_t *>(w + plan.hist2_at);
        // :41-43 oldPcm = Decode(adpcm, SampleCount = loopEnd) -> PcmAligned[0, loopEnd)
        if (int rc = gc::launch_decode(d_adpcm, adpcm_pitch, d_coefs, nch, p->loop_end, nullptr, nullptr, pcm, ppitch, nullptr, st))
            return rc;
        // :44-55 the tail to encode: rest of the last kept-from frame, then the loop, wrapped
        if (int rc = gc::launch_align_gather(pcm, ppitch, nch, p->loop_start, p->loop_end, plan.samples_to_keep, plan.samples_to_encode,
                                             new_pcm, plan.new_pitch, h1, h2, st))
            return rc;
        // :57-59 AdpcmAligned = kept frames + Encode(newPcm, history of the last kept sample)
        if (plan.bytes_to_keep > 0)
            VGA_HIP_TRY(hipMemcpy2DAsync(d_adpcm_out, (size_t)out_pitch, d_adpcm, (size_t)adpcm_pitch, (size_t)plan.bytes_to_keep,
                                         (size_t)nch, hipMemcpyDeviceToDevice, st));
        if (int rc = gc::launch_encode(new_pcm, plan.new_pitch, nch, plan.samples_to_encode, d_coefs, h1, h2,
                                       d_adpcm_out + plan.bytes_to_keep, out_pitch, st))
            return rc;
        // :61-62 PcmAligned[samplesToKeep..] = Decode(newAdpcm)
        if (int rc = gc::launch_decode(d_adpcm_out + plan.bytes_to_keep, out_pitch, d_coefs, nch, plan.samples_to_encode, h1, h2,
                                       pcm + plan.samples_to_keep, ppitch, nullptr, st))
            return rc;
    } else {
        if (d_adpcm_out && bytes_al > 0)
            VGA_HIP_TRY(hipMemcpy2DAsync(d_adpcm_out, (size_t)out_pitch, d_adpcm, (size_t)adpcm_pitch, (size_t)bytes_al,
                                         (size_t)nch, hipMemcpyDeviceToDevice, st));
        if (d_pcm_out || want_seek || ctx_needs_pcm)            // EnsurePcmDecoded (GcAdpcmChannelBuilder.cs:202)
            if (int rc = gc::launch_decode(d_adpcm, adpcm_pitch, d_coefs, nch, n_al, nullptr, nullptr, pcm, ppitch, nullptr, st))
                return rc;
    }
    return gc::launch_channel_meta(d_adpcm, adpcm_pitch, pcm, ppitch, nch, L.loop_start_aligned, p->samples_per_seek_table_entry,
                                   want_seek ? L.seek_table_entries : 0, want_seek ? d_seek_out : nullptr, seek_pitch,
                                   d_loop_context_out, st);
}

// GcAdpcmChannel(GcAdpcmChannelBuilder) for a batch of freshly encoded channels that share one loop
// (GcAdpcmFormat.cs:27-40): alignment re-encode, loop context, seek table.  Outputs may be null.
int vga_gcadpcm_build_channels_batch(const uint8_t *const *adpcm, const int16_t *coefs, int nch,
                                     const vga_gcadpcm_channel_params *p, uint8_t *const *adpcm_out,
                                     int16_t *const *pcm_out, int16_t *const *seek_table_out, int16_t *loop_context_out)
{
    vga_gcadpcm_channel_layout L;
    if (int rc = gc::channel_layout_for(p, &L)) return rc;
    if (int rc = gc::check_ptrs((const void *const *)adpcm, nch, "adpcm")) return rc;
    if (nch > 0 && !coefs) { set_error("null coefs"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (L.alignment_needed && !adpcm_out) { set_error("the loop needs alignment: adpcm_out is required"); return VGA_ERR_ARGUMENT; }
    if (adpcm_out) if (int rc = gc::check_ptrs((const void *const *)adpcm_out, nch, "adpcm_out")) return rc;
    if (pcm_out) if (int rc = gc::check_ptrs((const void *const *)pcm_out, L.sample_count_aligned > 0 ? nch : 0, "pcm_out")) return rc;
    if (seek_table_out && L.seek_table_entries > 0)
        if (int rc = gc::check_ptrs((const void *const *)seek_table_out, nch, "seek_table_out")) return rc;
    if (int rc = require_device()) return rc;
    gc::GcBatch b;
    VGA_HIP_TRY(b.st.create());
    const int bytes_in = gc::sample_count_to_byte_count(p->sample_count);
    const int bytes_al = gc::sample_count_to_byte_count(L.sample_count_aligned);
    const int64_t in_pitch = round_up(bytes_in > 0 ? bytes_in : 1, 16);
    b.adpcm_pitch = round_up(bytes_al > 0 ? bytes_al : 1, 16);
    b.pcm_pitch = round_up(L.sample_count_aligned > 0 ? L.sample_count_aligned : 1, 8);
    const int64_t seek_pitch = round_up(2 * (L.seek_table_entries > 0 ? L.seek_table_entries : 1), 8);
    DevBuf in, seek, ctx;
    VGA_HIP_TRY(in.alloc((size_t)nch * in_pitch));
    VGA_HIP_TRY(b.adpcm.alloc((size_t)nch * b.adpcm_pitch));
    VGA_HIP_TRY(b.pcm.alloc((size_t)nch * b.pcm_pitch * 2));
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    VGA_HIP_TRY(seek.alloc((size_t)nch * seek_pitch * 2));
    VGA_HIP_TRY(ctx.alloc((size_t)nch * 6));
    const size_t wsb = gc::build_channels_workspace_bytes(nch, p);
    VGA_HIP_TRY(b.ws.alloc(wsb));
    for (int c = 0; c < nch; c++)
        if (bytes_in > 0)
            VGA_HIP_TRY(hipMemcpyAsync(in.as<uint8_t>() + (int64_t)c * in_pitch, adpcm[c], (size_t)bytes_in,
                                       hipMemcpyHostToDevice, b.st.s));
    VGA_HIP_TRY(hipMemcpyAsync(b.coefs.p, coefs, (size_t)nch * 32, hipMemcpyHostToDevice, b.st.s));
    if (int rc = vga_gcadpcm_build_channels_device(in.as<uint8_t>(), in_pitch, b.coefs.as<int16_t>(), nch, p,
                                                   (adpcm_out || L.alignment_needed) ? b.adpcm.as<uint8_t>() : nullptr,
                                                   b.adpcm_pitch, pcm_out ? b.pcm.as<int16_t>() : nullptr, b.pcm_pitch,
                                                   (seek_table_out && L.seek_table_entries > 0) ? seek.as<int16_t>() : nullptr,
                                                   seek_pitch, loop_context_out ? ctx.as<int16_t>() : nullptr, b.ws.p, wsb, b.st.s))
        return rc;
    for (int c = 0; c < nch; c++)
        if (adpcm_out && bytes_al > 0)
            VGA_HIP_TRY(hipMemcpyAsync(adpcm_out[c], b.adpcm.as<uint8_t>() + (int64_t)c * b.adpcm_pitch, (size_t)bytes_al,
                                       hipMemcpyDeviceToHost, b.st.s));
    for (int c = 0; c < nch; c++) {
        if (pcm_out && L.sample_count_aligned > 0)
            VGA_HIP_TRY(hipMemcpyAsync(pcm_out[c], b.pcm.as<int16_t>() + (int64_t)c * b.pcm_pitch,
                                       (size_t)L.sample_count_aligned * 2, hipMemcpyDeviceToHost, b.st.s));
        if (seek_table_out && L.seek_table_entries > 0)
            VGA_HIP_TRY(hipMemcpyAsync(seek_table_out[c], seek.as<int16_t>() + (int64_t)c * seek_pitch,
                                       (size_t)L.seek_table_entries * 4, hipMemcpyDeviceToHost, b.st.s));
    }
    if (loop_context_out)
        VGA_HIP_TRY(hipMemcpyAsync(loop_context_out, ctx.p, (size_t)nch * 6, hipMemcpyDeviceToHost, b.st.s));
    VGA_HIP_TRY(hipStreamSynchronize(b.st.s));
    return VGA_OK;
}

// ---------------------------------------------------------------- DSP container
int vga_dsp_layout_for(const vga_dsp_params *p, int nch, vga_dsp_layout *out) { return gc::dsp_layout_for(p, nch, out); }

int vga_dsp_write_device(const uint8_t *d_adpcm, int64_t adpcm_pitch, int adpcm_len, const int16_t *d_coefs,
                         const int16_t *d_gain, const int16_t *d_start_context, const int16_t *d_loop_context, int nch,
                         const vga_dsp_params *p, uint8_t *d_file, void *stream)
{
    vga_dsp_layout L;
    if (int rc = gc::dsp_layout_for(p, nch, &L)) return rc;
    if (adpcm_len < 0 || !d_coefs || !d_file || (adpcm_len > 0 && !d_adpcm)) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (adpcm_len > 0)
        if (int rc = gc::check_adpcm_layout(d_adpcm, adpcm_pitch, adpcm_len, "vga_dsp_write_device")) return rc;
    if (((uintptr_t)d_file & 7) != 0) { set_error("file image must be 8-byte aligned"); return VGA_ERR_ARGUMENT; }
    const int mono_bytes = gc::sample_count_to_byte_count(L.sample_count);
    if (nch == 1 && mono_bytes > adpcm_len) {                   // Stream.Write(buffer, 0, count) past the array
        set_error("channel audio (%d bytes) is shorter than the %d bytes the header's sample count needs", adpcm_len, mono_bytes);
        return VGA_ERR_ARGUMENT;
    }
    return gc::launch_dsp_image(d_adpcm, adpcm_pitch, adpcm_len, d_coefs, d_gain, d_start_context, d_loop_context, nch,
                                L.sample_count, gc::sample_count_to_nibble_count(L.sample_count), p->sample_rate,
                                p->looping ? 1 : 0, L.start_addr, L.end_addr, L.cur_addr, L.bytes_per_interleave,
                                L.frames_per_interleave, L.audio_data_size, mono_bytes, d_file, (size_t)L.file_size,
                                (hipStream_t)stream);
}

// DspWriter.GetFile for channels held in host memory: the image is assembled on the device and copied back once.
int vga_dsp_write(const uint8_t *const *adpcm, int adpcm_len, const int16_t *coefs, const int16_t *gain,
                  const int16_t *start_context, const int16_t *loop_context, int nch, const vga_dsp_params *p,
                  uint8_t *file_out)
{
    vga_dsp_layout L;
    if (int rc = gc::dsp_layout_for(p, nch, &L)) return rc;
    if (adpcm_len < 0) { set_error("negative length"); return VGA_ERR_ARGUMENT; }
    if (int rc = gc::check_ptrs((const void *const *)adpcm, adpcm_len > 0 ? nch : 0, "adpcm")) return rc;
    if (!coefs || !file_out) { set_error("null coefs / output"); return VGA_ERR_ARGUMENT; }
    if (int rc = require_device()) return rc;
    gc::GcBatch b;
    VGA_HIP_TRY(b.st.create());
    b.adpcm_pitch = round_up(adpcm_len > 0 ? adpcm_len : 1, 16);
    DevBuf file, d_gain, d_sc, d_lc;
    VGA_HIP_TRY(b.adpcm.alloc((size_t)nch * b.adpcm_pitch));
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    VGA_HIP_TRY(file.alloc((size_t)L.file_size));
    for (int c = 0; c < nch; c++)
        if (adpcm_len > 0)
            VGA_HIP_TRY(hipMemcpyAsync(b.adpcm.as<uint8_t>() + (int64_t)c * b.adpcm_pitch, adpcm[c], (size_t)adpcm_len,
                                       hipMemcpyHostToDevice, b.st.s));
    VGA_HIP_TRY(hipMemcpyAsync(b.coefs.p, coefs, (size_t)nch * 32, hipMemcpyHostToDevice, b.st.s));
    auto upload = [&](DevBuf &d, const int16_t *src, size_t shorts) -> int {
        if (!src) return VGA_OK;
        VGA_HIP_TRY(d.alloc(shorts * 2));
        VGA_HIP_TRY(hipMemcpyAsync(d.p, src, shorts * 2, hipMemcpyHostToDevice, b.st.s));
        return VGA_OK;
    };
    if (int rc = upload(d_gain, gain, (size_t)nch)) return rc;
    if (int rc = upload(d_sc, start_context, (size_t)nch * 3)) return rc;
    if (int rc = upload(d_lc, loop_context, (size_t)nch * 3)) return rc;
    if (int rc = vga_dsp_write_device(b.adpcm.as<uint8_t>(), b.adpcm_pitch, adpcm_len, b.coefs.as<int16_t>(),
                                      gain ? d_gain.as<int16_t>() : nullptr, start_context ? d_sc.as<int16_t>() : nullptr,
                                      loop_context ? d_lc.as<int16_t>() : nullptr, nch, p, file.as<uint8_t>(), b.st.s))
        return rc;
    VGA_HIP_TRY(hipMemcpyAsync(file_out, file.p, (size_t)L.file_size, hipMemcpyDeviceToHost, b.st.s));
    VGA_HIP_TRY(hipStreamSynchronize(b.st.s));
    return VGA_OK;
}

}  // extern "C"
