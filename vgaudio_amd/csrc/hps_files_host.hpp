// hps_files_host.hpp -- the host side of include/vgaudio_hip_files/hps_files.h without HIP: every check, the packed layout of a
// set of HPS files (rows, images), the per-file table, the BLOCK TABLE of the whole set and the work items the kernels of
// hps_files_kernels.hip read, and the regions those items write (the testing hook).  File f of a set is what gcs::hps_layout
// (vga_hps_layout_for's and vga_hps_block_map's code) says for the file's numbers.  Header-only and free of
// <hip/hip_runtime.h>, so that a stand-alone host program can include it (tests/host/hps_files_host_driver.cpp) as
// capi_hps_files.hip does; whoever includes it supplies vga::set_error and vga::last_error.
#pragma once
#include "gc_files_host.hpp"
#include "gc_stream_host.hpp"
#include "../../include/vgaudio_hip_files/hps_files.h"

namespace vga {
namespace hpf {

using fileset::name_file;
constexpr uint32_t CHUNK_BYTES16 = 16384;        // of one work item of 16-byte granules: 256 threads, four granules each
constexpr uint32_t CHUNK_BYTES1 = 1024;          // of one work item of the general (byte) form of the gather

// What the kernels need of one file (a device table, one per file).  A set for reading fills image_off, first_channel, nch.
struct FileTab {
    int64_t image_off;
    int first_channel, nch, sample_rate, end_address, header_size, block_header_size;
};
// One block of one file: an entry of the set's block table, 32 bytes, roughly one per 64 KiB of image.
//   written: vga_hps_block's numbers; the body lies at image_off + offset + block_header_size
//   read:    channel c's audio_bytes at src + stride * c of the images go to out_offset of row first_channel + c
struct Block {
    union {
        struct { int file, offset, next_offset, written_size, end_nibble, start_sample, byte_in_index, channel_size; } w;
        struct { int64_t src; int stride, audio_bytes, out_offset, first_channel, file, granule; } r;
    };
};
static_assert(sizeof(Block) == 32, "block table entry");
struct Row { int64_t pcm_off, adpcm_off; };      // of the ragged batch
// a work item: bytes [start, end) of block `block`'s body (write) or of its audio of row `row` (read)
struct Item { int block, row; uint32_t start, end; };
struct ChannelMeta { int16_t v[23]; };           // the reader's per-channel arrays as the object holds them (fileset::fill_meta)

struct FilesLayout {
    vga_hps_files_totals totals = {};
    bool from_infos = false;
    std::vector<vga_hps_layout> layout;          // per file (a set for writing)
    std::vector<int> sample_rate, nch;           // per file
    std::vector<int> first_channel, counts;      // per file; per channel (the ragged batch's sample counts)
    std::vector<int64_t> image_off, first_block; // per file
    std::vector<int> image_size;                 // per file
    gc::RaggedLayout rows;
    std::vector<Row> channel;
    std::vector<ChannelMeta> meta;               // (from_infos)
    std::vector<FileTab> tab;
    std::vector<Block> blocks;
    std::vector<Item> items;
};

inline vga_hps_params params_of(const vga_hps_file &F) { return {F.sample_rate, F.sample_count, F.looping, F.loop_start, F.loop_end}; }

// a fresh layout with its per-file arrays
inline void start_layout(FilesLayout &L, int nfiles, bool from_infos)
{
    fileset::start_layout(L, nfiles, from_infos);
    L.sample_rate.resize(nfiles);
    L.nch.resize(nfiles);
    L.first_block.resize(nfiles);
}

inline int check_counts(const FilesLayout &L, int f)
{
    if ((int64_t)L.blocks.size() + L.totals.files > 0x7FFFFFFF || L.items.size() > (size_t)0x7FFFFFFF) {
        set_error("file %d: more than 2^31 blocks or work items in one set", f);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

inline int make_layout(const vga_hps_file *files, int nfiles, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    start_layout(L, nfiles, false);
    L.layout.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    std::vector<vga_hps_block> map;
    for (int f = 0; f < nfiles; f++) {
        const vga_hps_file &F = files[f];
        const vga_hps_params p = params_of(F);
        vga_hps_layout &N = L.layout[f];
        if (int rc = gcs::hps_layout(&p, F.channels, &N, &map)) return name_file(f, rc);
        vga_gcadpcm_channel_layout cl;
        if (int rc = gc::channel_layout_for(&N.channel, &cl)) return name_file(f, rc);
        // the rows are the aligned set's: cl.sample_count_aligned samples of PCM, channel_adpcm_bytes of ADPCM
        if (int rc = gcs::hps_check_pcm(map, cl.sample_count_aligned)) return name_file(f, rc);
        if ((int64_t)map.back().byte_in_index + map.back().channel_size > N.channel_adpcm_bytes) {
            set_error("file %d: internal: the block map reaches past the row", f);
            return VGA_ERR_INVALID_OP;
        }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, F.channels, channels, "channels")) return rc;
        const fileset::Placed image = images.place(N.file_size);
        L.sample_rate[f] = F.sample_rate;
        L.nch[f] = F.channels;
        L.first_channel[f] = first;
        L.first_block[f] = (int64_t)L.blocks.size();
        for (int i = 0; i < F.channels; i++) L.counts.push_back(cl.sample_count_aligned);
        L.tab[f] = {image.at, first, F.channels, F.sample_rate, gc::sample_to_nibble(N.sample_count - 1), N.header_size,
                    N.block_header_size};
        for (const vga_hps_block &b : map) {
            Block B;
            B.w = {f, b.offset, b.next_offset, b.written_size, b.end_nibble, b.start_sample, b.byte_in_index, b.channel_size};
            const int at = (int)L.blocks.size();
            L.blocks.push_back(B);
            for (uint32_t s = 0; s < (uint32_t)b.written_size; s += CHUNK_BYTES16)
                L.items.push_back({at, 0, s, std::min(s + CHUNK_BYTES16, (uint32_t)b.written_size)});
        }
        if (int rc = check_counts(L, f)) return rc;
        L.image_off[f] = image.at;
        L.image_size[f] = N.file_size;
        if (image.verdict & fileset::TOTAL_PAST_MAX) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    }
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.image_bytes = images.total();
    L.totals.blocks = (int64_t)L.blocks.size();
    return VGA_OK;
}

// a set for reading, from what vga_hps_parse returned for every file
inline int make_layout_from_infos(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file, int nfiles,
                                  const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos && blocks_per_file, "infos / block tables")) return rc;
    start_layout(L, nfiles, true);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_hps_info *I = infos[f];
        const vga_hps_block_info *blocks = blocks_per_file[f];
        if (!I || !blocks) { set_error("file %d: null info / block table", f); return VGA_ERR_ARGUMENT; }
        if (int rc = gcs::hps_check_info(I)) return name_file(f, rc);           // vga_hps_read_device's checks, codes and messages
        const int nch = I->channel_count;
        // the set's own: the rows are the header's (what vga_hps_parse fills for a file HpsWriter wrote passes)
        if (I->sample_count < 0 || I->adpcm_bytes != gc::sample_count_to_byte_count(I->sample_count)) {
            set_error("file %d: the info's rows of %d bytes are not those of its %d samples", f, I->adpcm_bytes, I->sample_count);
            return VGA_ERR_ARGUMENT;
        }
        // the image's size is known once its blocks are: it is placed behind them, where it lies is needed in front
        const int64_t at = image_offsets ? image_offsets[f] : images.at;
        if (at < 0) { set_error("file %d: negative image offset %lld", f, (long long)at); return VGA_ERR_ARGUMENT; }
        if (at > fileset::MAX_TOTAL) { set_error("file %d: image offset past 2^62", f); return VGA_ERR_OUT_OF_RANGE; }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, nch, channels, "channels")) return rc;
        L.sample_rate[f] = I->sample_rate;
        L.nch[f] = nch;
        L.first_channel[f] = first;
        L.first_block[f] = (int64_t)L.blocks.size();
        L.image_off[f] = at;
        L.tab[f] = {at, first, nch, I->sample_rate, 0, 0, 0};
        int64_t size = 0;
        for (int i = 0; i < I->block_count; i++) {
            const vga_hps_block_info &b = blocks[i];
            if (int rc = gcs::hps_check_block(I, b, i)) return name_file(f, rc);
            if (b.audio_offset < 0 || b.size < 0) { set_error("file %d: block %d lies at a negative offset", f, i); return VGA_ERR_ARGUMENT; }
            const int stride = b.size / nch;
            // the image reaches to the end of its last block, as a written file does, and holds every channel's audio
            size = std::max({size, (int64_t)b.audio_offset + b.size, (int64_t)b.audio_offset + (int64_t)stride * (nch - 1) + b.audio_bytes});
            Block B;
            const uint64_t geometry = (uint64_t)(at + b.audio_offset) | (uint64_t)stride | (uint64_t)b.out_offset;
            B.r = {at + b.audio_offset, stride, b.audio_bytes, b.out_offset, first, f, geometry % 16 == 0 ? 16 : 1};
            const int blk = (int)L.blocks.size();
            L.blocks.push_back(B);
            const uint32_t step = B.r.granule == 16 ? CHUNK_BYTES16 : CHUNK_BYTES1;
            for (int c = 0; c < nch; c++)
                for (uint32_t s = 0; s < (uint32_t)b.audio_bytes; s += step)
                    L.items.push_back({blk, first + c, s, std::min(s + step, (uint32_t)b.audio_bytes)});
        }
        if (int rc = check_counts(L, f)) return rc;
        if (images.place(size, &at).verdict & fileset::IMAGE_PAST_2GIB) { set_error("file %d: image past 2 GiB", f); return VGA_ERR_OUT_OF_RANGE; }
        L.image_size[f] = (int)size;
        for (int c = 0; c < nch; c++) {
            L.counts.push_back(I->sample_count);
            L.meta.push_back(fileset::fill_meta<ChannelMeta>(*I, c));
        }
    }
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.image_bytes = images.total();
    L.totals.blocks = (int64_t)L.blocks.size();
    return VGA_OK;
}

// ---- what the kernels write: the hook of hps_files.h
inline void regions_of(const FilesLayout &L, std::vector<vga_hps_files_region> &out)
{
    out.clear();
    if (L.from_infos) {
        for (const Item &it : L.items) out.push_back({VGA_HPS_FILES_AUDIO, it.row, L.blocks[it.block].r.granule,
                                                      (int64_t)L.blocks[it.block].r.out_offset + it.start,
                                                      (int64_t)L.blocks[it.block].r.out_offset + it.end});
        return;
    }
    for (int f = 0; f < L.totals.files; f++) out.push_back({VGA_HPS_FILES_HEADER, f, 0, 0, L.tab[f].header_size});
    for (const Block &B : L.blocks)
        out.push_back({VGA_HPS_FILES_BLOCK_HEADER, B.w.file, 0, B.w.offset, (int64_t)B.w.offset + L.tab[B.w.file].block_header_size});
    for (const Item &it : L.items) {
        const Block &B = L.blocks[it.block];
        const int64_t body = (int64_t)B.w.offset + L.tab[B.w.file].block_header_size;
        out.push_back({VGA_HPS_FILES_AUDIO, B.w.file, 16, body + it.start, body + it.end});
    }
}
inline int copy_regions(const FilesLayout &L, vga_hps_files_region *regions_out, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_hps_files_region> r;
    regions_of(L, r);
    return fileset::copy_regions(r, regions_out, capacity, count_out);
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_pcm, const void *d_images)
{
    const char *what = "vga_hps_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_hps_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_adpcm || !d_coefs || !d_images) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_pcm) || !gcf::aligned16(d_images)) {
        set_error("%s: d_adpcm, d_pcm and d_images need 16-byte alignment", what);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_adpcm)
{
    const char *what = "vga_hps_read_device_v";
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_hps_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || !d_adpcm) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace hpf
}  // namespace vga
