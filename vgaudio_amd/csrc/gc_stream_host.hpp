// gc_stream_host.hpp -- the host side of the HPS and IDSP writers (gc_containers.hip, idsp_files_host.hpp) without HIP: the
// channel-count check, HpsWriter.SetupWriter / CreateBlockMap (hps_layout) and IdspWriter's size math (idsp_layout).
// vga_hps_layout_for, vga_hps_block_map and vga_idsp_layout_for ARE these functions.  Header-only and free of
// <hip/hip_runtime.h>, so that a stand-alone host program can include it (tests/host/idsp_files_host_driver.cpp); whoever
// includes it supplies vga::set_error.
#pragma once
#include "container_math.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace vga {
namespace gcs {

using namespace vga::container;

constexpr int kMaxChannels = VGA_GC_CONTAINER_MAX_CHANNELS;
constexpr int kHpsMaxBlockSize = 0x10000;                   // HpsWriter.MaxBlockSize, written for every channel count
constexpr int kIdspStreamInfoSize = 0x40, kIdspChannelInfoSize = 0x60;   // IdspWriter.cs:33-34

inline int check_channels(int nch)
{
    if (nch < 1) { set_error("channel count %d: at least one channel", nch); return VGA_ERR_ARGUMENT; }
    if (nch > kMaxChannels) { set_error("%d channels: at most %d are written here", nch, kMaxChannels); return VGA_ERR_INVALID_OP; }
    return VGA_OK;
}

// HpsWriter.SetupWriter (:26-47) and CreateBlockMap (:114-160)
inline int hps_layout(const vga_hps_params *p, int nch, vga_hps_layout *L, std::vector<vga_hps_block> *map)
{
    if (!p || !L) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(L, 0, sizeof *L);
    if (int rc = check_channels(nch)) return rc;
    if (nch % 4 == 3) {
        set_error("HPS with %d channels: the reference counts a block header of 4 + 8 * %d bytes but writes 12 + 8 * %d, "
                  "one 0x20 line more than counted, and its writes overrun the image; it cannot write 3, 7, 11, ... channels",
                  nch, nch, nch);
        return VGA_ERR_INVALID_OP;
    }
    if (p->sample_rate < 0) return out_of_range("negative sample rate");
    if (int rc = check_loop(p->looping, p->loop_start, p->loop_end, p->sample_count)) return rc;
    const int loop_start = p->looping ? p->loop_start : 0, loop_end = p->looping ? p->loop_end : 0;
    L->header_size = (int)next_multiple(std::max(0x80, 0x10 + 0x38 * nch), 0x20);
    L->channel_size = (int)next_multiple(kHpsMaxBlockSize / nch, 0x20);
    const int max_block_size_actual = L->channel_size * nch;
    L->alignment = gc::byte_count_to_sample_count(L->channel_size);
    // WithAlignment when the loop start is not aligned, then every channel rebuilt with LoopAlignmentMultiple
    L->channel.sample_count = p->sample_count;
    L->channel.looping = p->looping ? 1 : 0;
    L->channel.loop_start = loop_start;
    L->channel.loop_end = loop_end;
    L->channel.loop_alignment_multiple = L->alignment;
    vga_gcadpcm_channel_layout cl;
    if (int rc = gc::channel_layout_for(&L->channel, &cl)) return rc;
    L->alignment_needed = cl.alignment_needed;
    const int shift = cl.alignment_needed ? cl.loop_start_aligned - loop_start : 0;            // GcAdpcmFormat.cs:15-18
    L->looping = p->looping ? 1 : 0;
    L->loop_start = loop_start + shift;
    L->loop_end = loop_end + shift;
    L->sample_count = shift == 0 ? p->sample_count : L->loop_end;
    L->channel_adpcm_bytes = bytes_of(cl.sample_count_aligned);
    L->block_header_size = (int)next_multiple(12 + 8 * nch, 0x20);
    const int counted_header = (int)next_multiple(4 + 8 * nch, 0x20);                          // BlockInfo.TotalSize (:179)
    // CreateBlockMap
    const int nibble_count = gc::sample_count_to_nibble_count(L->sample_count);
    const int max_channel_block = max_block_size_actual / nch * 2;
    const int block_count = div_round_up(nibble_count, max_channel_block);
    if (block_count == 0) return out_of_range("an HPS file needs at least one block: the reference indexes blocks[0] of an empty map");
    const int loop_block = L->looping ? gc::sample_to_nibble(L->loop_start) / max_channel_block : block_count - 1;
    std::vector<vga_hps_block> local;
    std::vector<vga_hps_block> &m = map ? *map : local;
    m.assign((size_t)block_count, vga_hps_block{});
    auto block = [&](int at, int nibble, int size) {
        vga_hps_block &b = m[at];
        b.start_sample = gc::nibble_to_sample(nibble + 2);           // the predictor / scale nibbles are not samples
        b.byte_in_index = nibble / 2;
        b.end_nibble = size - 1;
        b.channel_size = size / 2 + (size & 1);
        b.written_size = (int)next_multiple(b.channel_size, 0x20) * nch;
        b.total_size = counted_header + b.written_size;
    };
    int nibble = 0, at = 0;
    for (; at < loop_block; at++, nibble += max_channel_block) block(at, nibble, max_channel_block);
    while (nibble < nibble_count) {
        if (at >= block_count) { set_error("HPS block map overflow"); return VGA_ERR_INVALID_OP; }   // not reached
        const int left = nibble_count - nibble;
        const int size = std::min(left, (int)next_multiple(div_round_up(left, block_count - at), 0x40));
        block(at++, nibble, size);
        nibble += size;
    }
    if (at != block_count) { set_error("HPS block map underflow"); return VGA_ERR_INVALID_OP; }      // not reached
    int64_t offset = L->header_size;
    for (int i = 0; i < block_count; i++) {
        m[i].offset = (int)std::min<int64_t>(offset, 0x7FFFFFFF);
        offset += m[i].total_size;
    }
    if (offset > 0x7FFFFFFF) return out_of_range("file would exceed 2 GiB (the reference's FileSize is an int)");
    for (int i = 0; i + 1 < block_count; i++) m[i].next_offset = m[i + 1].offset;
    m[block_count - 1].next_offset = L->looping ? m[loop_block].offset : -1;
    L->block_count = block_count;
    L->loop_block = loop_block;
    L->file_size = (int)offset;
    return VGA_OK;
}

// GetHist1 / GetHist2 index Pcm[StartSample - 1 / - 2] of rows of pcm_len samples (vga_hps_write_device; a set's create)
inline int hps_check_pcm(const std::vector<vga_hps_block> &map, int pcm_len)
{
    for (const vga_hps_block &b : map)
        if (b.start_sample >= 1 && b.start_sample - 1 >= pcm_len) {
            set_error("block at sample %d reads hist1 at Pcm[%d] of %d samples (IndexOutOfRangeException)", b.start_sample,
                      b.start_sample - 1, pcm_len);
            return VGA_ERR_OUT_OF_RANGE;
        }
    return VGA_OK;
}

// what vga_hps_read_device asks of a parsed file and of block i of its table (a set's create asks the same)
inline int hps_check_info(const vga_hps_info *I)
{
    const int nch = I->channel_count;
    if (nch < 1 || nch > kMaxChannels || I->block_count < 1) { set_error("info does not describe an HPS file"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int hps_check_block(const vga_hps_info *I, const vga_hps_block_info &b, int i)
{
    if (b.audio_bytes < 0 || b.out_offset < 0 || (int64_t)b.out_offset + b.audio_bytes > I->adpcm_bytes) {
        set_error("block %d does not fit the info", i);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

// what vga_idsp_read_device asks of a parsed file (a set's create asks the same)
inline int idsp_check_info(const vga_idsp_info *I)
{
    const int nch = I->channel_count;
    if (nch < 1 || nch > kMaxChannels || I->interleave <= 0 || I->audio_data_length < 0 || I->adpcm_bytes < 0) {
        set_error("info does not describe an IDSP file");
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

// IdspWriter (:17-51)
inline int idsp_layout(const vga_idsp_params *p, int nch, vga_idsp_layout *L)
{
    if (!p || !L) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(L, 0, sizeof *L);
    if (int rc = check_channels(nch)) return rc;
    if (p->block_size < 0) return out_of_range("Number of samples per interleave must be non-negative");   // IdspConfiguration.cs
    if (p->block_size % 8 != 0) return out_of_range("Number of samples per interleave must be divisible by 14");  // sic: % BytesPerFrame
    if (p->sample_rate < 0) return out_of_range("negative sample rate");
    if (int rc = check_loop(p->looping, p->loop_start, p->loop_end, p->sample_count)) return rc;
    const int loop_start = p->looping ? p->loop_start : 0, loop_end = p->looping ? p->loop_end : 0;
    L->channel.sample_count = p->sample_count;
    L->channel.looping = p->looping ? 1 : 0;
    L->channel.loop_start = loop_start;
    L->channel.loop_end = loop_end;
    L->channel.loop_alignment_multiple = p->block_size ? gc::byte_count_to_sample_count(p->block_size) : 0;
    vga_gcadpcm_channel_layout cl;
    if (int rc = gc::channel_layout_for(&L->channel, &cl)) return rc;
    L->alignment_needed = cl.alignment_needed;
    L->channel_sample_count = cl.sample_count_aligned;
    L->channel_adpcm_bytes = bytes_of(cl.sample_count_aligned);
    const int shift = cl.alignment_needed ? cl.loop_start_aligned - loop_start : 0;
    L->looping = p->looping ? 1 : 0;
    L->loop_start = loop_start + shift;
    L->loop_end = loop_end + shift;
    const int format_samples = shift == 0 ? p->sample_count : L->loop_end;
    L->sample_count = p->trim_file && L->looping ? L->loop_end : std::max(format_samples, L->loop_end);
    L->start_addr = gc::sample_to_nibble(L->looping ? L->loop_start : 0);
    L->end_addr = gc::sample_to_nibble(L->looping ? L->loop_end : L->sample_count - 1);
    L->cur_addr = gc::sample_to_nibble(0);
    L->audio_data_size = (int)next_multiple(bytes_of(L->sample_count), p->block_size == 0 ? 8 : p->block_size);
    L->interleave_size = p->block_size == 0 ? L->audio_data_size : p->block_size;
    if (L->interleave_size == 0) {
        set_error("IDSP without audio and with BlockSize 0: the reference's Interleave divides by the zero interleave size");
        return VGA_ERR_INVALID_OP;
    }
    L->header_size = kIdspStreamInfoSize + kIdspChannelInfoSize * nch;
    const int64_t file = L->header_size + (int64_t)L->audio_data_size * nch;
    if (file > 0x7FFFFFFF) return out_of_range("file would exceed 2 GiB (the reference's FileSize is an int)");
    L->file_size = (int)file;
    return VGA_OK;
}

}  // namespace gcs
}  // namespace vga
