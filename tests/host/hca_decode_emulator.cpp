// hca_decode_emulator.cpp -- host-side lane emulator of the two HCA decoder launches, built from the SAME header the
// kernels use (vgaudio_amd/csrc/hca_decode_core.hpp).  TEST ONLY: lets the CPU suite hold the scan's bit walk, the
// chunk decoder, the 8-lane DCT-IV decomposition, the row rotation and the overlap carry of hca_frames_kernel to the
// oracle without a GPU.  Compiled by tests/test_host_hca_decode_core.py.  The "threads" of a workgroup are run one
// after the other, phase by phase, exactly where the kernel has its barriers.
#include <cstring>
#include <vector>

#define HCA_TABLE_QUAL static const
#include "../../vgaudio_amd/csrc/hca_tables_data.h"
#include "../../vgaudio_amd/csrc/hca_decode_core.hpp"

using namespace vga::hca;

namespace {

struct Tab {
    Symbol sym[16];
    uint8_t curve[64];
    Tab()
    {
        for (int r = 0; r < 16; r++)
            sym[r] = make_symbol(r, HCA_QuantizedSpectrumBits[r & 7], HCA_QuantizedSpectrumValue[r & 7], HCA_QuantizedSpectrumMaxBits[r]);
        for (int i = 0; i < 64; i++) curve[i] = i < 59 ? HCA_ScaleToResolutionCurve[i] : 0;
    }
    const Symbol &symbol(int r) const { return sym[r]; }
    uint64_t symbol_len(int r) const { return sym[r].len; }
    const uint8_t *res_curve() const { return curve; }
};

struct Src {
    const uint8_t *stream;             // the stream's frames
    int64_t w0, limit;                 // first aligned dword of the frame, dwords readable from there
    uint32_t word(int64_t k) const
    {
        uint32_t v;
        std::memcpy(&v, stream + 4 * (w0 + (k < limit ? k : limit - 1)), 4);
        return v;
    }
    void quad(int64_t k, uint32_t out[4]) const
    {
        for (int e = 0; e < 4; e++) out[e] = word(k + e);
    }
};
struct Ring {
    uint32_t v[16];
    void put(int s, uint32_t x) { v[s] = x; }
    uint32_t get(int s) const { return v[s]; }
};
struct Res {
    uint32_t v[8][16];
    void put(int c, int w, uint32_t x) { v[c][w] = x; }
    uint32_t get(int c, int w) const { return v[c][w]; }
};
struct Out {
    uint8_t *rec;
    int at = 0;
    void piece(const uint32_t p[4])
    {
        std::memcpy(rec + at, p, 16);
        at += 16;
    }
};
struct FB {
    const uint32_t *w;
    int zero_at;
    uint32_t get(int k) const { return w[k < zero_at ? k : zero_at]; }
};
struct Res16 {
    uint8_t b[16];
    int operator[](int e) const { return b[e]; }
};

}  // namespace

extern "C" {

int emu_record_bytes(const DeviceInfo *info) { return make_decode_layout(*info).record_bytes; }

// the scan of every frame of one stream: records[frame_count][record_bytes]; returns the OR of the frames' flags
int emu_hca_scan(const DeviceInfo *info, const uint8_t *stream, int64_t pitch, uint8_t *records)
{
    const DecodeLayout lay = make_decode_layout(*info);
    static const Tab tab;
    int all = 0;
    for (int f = 0; f < info->frame_count; f++) {
        const int64_t a0 = (int64_t)f * info->frame_size;
        Src src{stream, a0 >> 2, pitch / 4 - (a0 >> 2)};
        Ring ring{};
        Res res{};
        Out out{records + (size_t)f * lay.record_bytes};
        ScanParams P{info->nch, info->frame_size * 8, (int)(a0 & 3) * 8, info->hfr_group_count, info->coded_count,
                     info->channel_type, info->ath_curve, lay.wide_offsets, info->stereo_band_count > 0};
        all |= scan_frame(P, src, ring, res, out, tab);
        if (out.at > lay.record_bytes) return -1;
    }
    return all;
}

// hca_frames_kernel for one stream: pcm[nch][pcm_pitch]
int emu_hca_frames(const DeviceInfo *info, const uint8_t *stream, int64_t pitch, const uint8_t *records, int16_t *pcm,
                   int64_t pcm_pitch, int frames_per_group)
{
    const DecodeLayout lay = make_decode_layout(*info);
    static const Tab tab;
    const int nch = info->nch, NT = 128;
    std::vector<char> rows((size_t)nch * 9 * ROW_BYTES);
    std::vector<double> gain((size_t)nch * 128);
    std::vector<uint8_t> resb((size_t)nch * 128);
    std::vector<uint32_t> fbw(lay.frame_dwords + 1);
    double window[128];
    for (int i = 0; i < 128; i++) {
        float w;
        std::memcpy(&w, &HCA_MdctWindowF32Bits[i], 4);
        window[i] = (double)w;
    }
    DctLane K[8];
    for (int L = 0; L < 8; L++) K[L] = make_dct_lane(MDCT_SinBits, MDCT_CosBits, L);
    const DctUniform U = make_dct_uniform(MDCT_SinBits, MDCT_CosBits);
    const int F = frames_per_group > 0 ? frames_per_group : 1;

    for (int f0 = 0; f0 < info->frame_count; f0 += F) {
        const int f1 = f0 + F < info->frame_count ? f0 + F : info->frame_count;
        std::memset(rows.data(), 0x55, rows.size());                      // a fresh workgroup: LDS holds garbage
        for (int f = f0 > 0 ? f0 - 1 : f0; f < f1; f++) {
            const bool warm = f < f0;
            const int base = (9 - f % 9) % 9;
            auto row_of = [&](int c, int sf) { return rows.data() + (size_t)(c * 9 + (base + sf) % 9) * ROW_BYTES; };
            auto prev_of = [&](int c) { return rows.data() + (size_t)(c * 9 + (base + 8) % 9) * ROW_BYTES; };
            const uint8_t *rec = records + (size_t)f * lay.record_bytes;
            // the frame's bytes as big-endian dwords, zero past its end
            const int64_t a0 = (int64_t)f * info->frame_size;
            const int64_t w0 = a0 >> 2, last = pitch / 4 - 1;
            const int sh8 = (int)(a0 & 3) * 8;
            for (int k = 0; k <= lay.frame_dwords; k++) {
                uint32_t v = 0;
                if (k < lay.frame_dwords) {
                    uint32_t x0, x1;
                    std::memcpy(&x0, stream + 4 * (w0 + k < last ? w0 + k : last), 4);
                    std::memcpy(&x1, stream + 4 * (w0 + k + 1 < last ? w0 + k + 1 : last), 4);
                    x0 = bswap32(x0);
                    x1 = bswap32(x1);
                    v = sh8 ? (x0 << sh8) | (x1 >> (32 - sh8)) : x0;
                    v = mask_past_end(v, k, info->frame_size * 8);
                }
                fbw[k] = v;
            }
            uint32_t head;
            std::memcpy(&head, rec + lay.header_at, 4);
            const int noise = head & 0xFFFF, eval = (head >> 16) & 0xFF;
            for (int b = 0; b < nch * 128; b++) {
                const int c = b >> 7, s = b & 127;
                const int sf = rec[c * REC_CHANNEL_BYTES + s];
                const int rs = s < info->coded_count[c] ? resolution_for(tab.res_curve(), sf, info->ath_curve[s] + noise - (s < eval ? 1 : 0)) : 0;
                resb[b] = (uint8_t)rs;
                gain[b] = bits_to_double(HCA_DequantizerScalingTableBits[sf]) * bits_to_double(HCA_QuantizerStepSizeBits[rs]);
            }
            if (f == 0)
                for (int c = 0; c < nch; c++) std::memset(prev_of(c), 0, ROW_BYTES);
            // stage A
            for (int id = 0; id < nch * 64; id++) {
                const int row = id >> 3, q = id & 7, c = row >> 3, sf = row & 7;
                if (warm && sf != 7) continue;
                int nsym = info->coded_count[c] - 16 * q;
                nsym = nsym < 0 ? 0 : (nsym > 16 ? 16 : nsym);
                uint32_t off = 0;
                if (nsym > 0) {
                    const int k = sf * lay.chunks_per_subframe + lay.chunk_base[c] + q;
                    if (lay.wide_offsets) std::memcpy(&off, rec + lay.offsets_at + 4 * k, 4);
                    else { uint16_t o16; std::memcpy(&o16, rec + lay.offsets_at + 2 * k, 2); off = o16; }
                }
                Res16 r16;
                std::memcpy(r16.b, &resb[c * 128 + 16 * q], 16);
                decode_chunk(FB{fbw.data(), lay.frame_dwords}, (int)off, nsym, 16 * q, r16, &gain[c * 128 + 16 * q], tab, row_of(c, sf));
            }
            // ReconstructHighFrequency (CriHcaDecoder.cs:116-145)
            if (info->hfr_group_count > 0) {
                const int total_band_count = info->total_band_count < 127 ? info->total_band_count : 127;
                const int hfr_start = info->base_band_count + info->stereo_band_count;
                int hfr_bands = total_band_count - info->hfr_band_count;
                if (info->hfr_band_count < hfr_bands) hfr_bands = info->hfr_band_count;
                for (int c = 0; c < nch; c++) {
                    if (info->channel_type[c] == CH_STEREO_SECONDARY) continue;
                    for (int sf = 0; sf < 8; sf++) {
                        if (warm && sf != 7) continue;
                        for (int band = 0; band < hfr_bands; band++) {
                            const int group = band / info->bands_per_hfr_group;
                            if (group >= info->hfr_group_count) continue;
                            const int high = hfr_start + band, low = hfr_start - band - 1;
                            const int index = (int)rec[c * REC_CHANNEL_BYTES + 136 + group] - (int)rec[c * REC_CHANNEL_BYTES + low] + 64;
                            char *r = row_of(c, sf);
                            *reinterpret_cast<double *>(r + spec_byte_offset(high)) =
                                bits_to_double(HCA_ScaleConversionTableBits[index & 127]) * *reinterpret_cast<double *>(r + spec_byte_offset(low));
                        }
                    }
                }
            }
            // ApplyIntensityStereo (:147-166)
            if (info->stereo_band_count > 0) {
                for (int c = 0; c < nch; c++) {
                    if (info->channel_type[c] != CH_STEREO_PRIMARY) continue;
                    for (int sf = 0; sf < 8; sf++) {
                        if (warm && sf != 7) continue;
                        const int iq = rec[(c + 1) * REC_CHANNEL_BYTES + 128 + sf];
                        const double ratio_l = bits_to_double(HCA_IntensityRatioTableBits[iq < 14 ? iq : 14]);
                        const double ratio_r = ratio_l - 2.0;
                        for (int b = info->base_band_count; b < info->total_band_count; b++) {
                            double *l = reinterpret_cast<double *>(row_of(c, sf) + spec_byte_offset(b));
                            double *r = reinterpret_cast<double *>(row_of(c + 1, sf) + spec_byte_offset(b));
                            const double lv = *l;
                            *r = lv * ratio_r;
                            *l = lv * ratio_l;
                        }
                    }
                }
            }
            // stage B: per transform, its eight lanes phase by phase
            for (int row = 0; row < nch * 8; row++) {
                const int c = row >> 3, sf = row & 7;
                if (warm && sf != 7) continue;
                char *r = row_of(c, sf);
                for (int L = 0; L < 8; L++) dct_first_half(r, L, K[L]);
                double y[8][16];
                for (int L = 0; L < 8; L++) dct_second_half(r, L, U, y[L]);
                for (int L = 0; L < 8; L++) dct_store(r, K[L], y[L]);
            }
            // stage C
            if (!warm) {
                for (int c = 0; c < nch; c++)
                    for (int sf = 0; sf < 8; sf++)
                        for (int j = 0; j < NT; j++) {
                            const double *cur = reinterpret_cast<const double *>(row_of(c, sf));
                            const double *prv = reinterpret_cast<const double *>(sf ? row_of(c, sf - 1) : prev_of(c));
                            const int sample = imdct_sample(j < 64, window[j], window[127 - j], cur[imdct_cur_index(j)], prv[imdct_prev_index(j)]);
                            const int64_t tpos = (int64_t)f * SPF + sf * SPSF + j - info->inserted_samples;
                            if (tpos >= 0 && tpos < info->sample_count) pcm[(int64_t)c * pcm_pitch + tpos] = (int16_t)sample;
                        }
            }
        }
    }
    return 0;
}

}  // extern "C"
