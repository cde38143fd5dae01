// gc_files_layout.hpp -- what the sets of the GC-ADPCM family (gc_files, gc_aligned, nw_files, hps_files, idsp_files) share
// below the object, on top of files_layout.hpp: the rows of the ragged batch, the seek tables behind one
// another and the per-channel metadata of a set for reading.  Header-only and free of <hip/hip_runtime.h>.
#pragma once
#include "files_layout.hpp"
#include "gc_host.hpp"

namespace vga {
namespace fileset {

// the packed rows of `counts` samples each: channel[c].pcm_off / adpcm_off and the sizes of the row buffers, guards included
template <class Row, class Totals>
inline void lay_out_rows(gc::RaggedLayout &rows, const std::vector<int> &counts, std::vector<Row> &channel, Totals &totals)
{
    const int nch = (int)counts.size();
    rows.lay_out(counts.data(), nch, 0, 0);
    channel.resize(nch);
    for (int c = 0; c < nch; c++) {
        channel[c].pcm_off = rows.pcm_off[c];
        channel[c].adpcm_off = rows.adpcm_off[c];
    }
    totals.channels = nch;
    totals.pcm_samples = rows.pcm_end + gc::GUARD_BYTES / 2;
    totals.adpcm_bytes = rows.adpcm_end + gc::GUARD_BYTES;
}
// channel[c].seek_off of tables of channel[c].entries shorts, each in room padded to 8 bytes; returns the shorts of all
template <class Row> inline int64_t lay_out_seek(std::vector<Row> &channel)
{
    int64_t seek_at = 0;
    for (Row &r : channel) {
        r.seek_off = seek_at;
        seek_at += pad_to(2 * (int64_t)r.entries, 8);
    }
    return seek_at;
}

// The reader's per-channel arrays as an object holds them, 23 shorts: 16 coefficients, the gain, start and loop context of
// three each.  Meta is the format's own `struct ChannelMeta { int16_t v[23]; }`: a kernel's signature names it.
template <class Meta, class Info> inline Meta fill_meta(const Info &I, int c)
{
    static_assert(sizeof(Meta) == 46 && sizeof(I.coefs[c]) == 32 && sizeof(I.start_context[c]) == 6 && sizeof(I.loop_context[c]) == 6,
                  "the meta kernels read 23 shorts");
    Meta m;
    std::memcpy(m.v, I.coefs[c], 32);
    m.v[16] = I.gain[c];
    std::memcpy(m.v + 17, I.start_context[c], 6);
    std::memcpy(m.v + 20, I.loop_context[c], 6);
    return m;
}

}  // namespace fileset
}  // namespace vga
