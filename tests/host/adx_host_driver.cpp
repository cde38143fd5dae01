// adx_host_driver.cpp -- vgaudio_amd/csrc/adx_host.hpp on its own (tests/test_adx_ragged_device_host.py): the header with a
// set_error of this file's, no HIP and no product library.  Built with g++, AddressSanitizer and UBSan, it runs a file of
// cases the test wrote from its own model of the layout and the plan:
//   int32 n; n x { int32 params[8] (the fields of vga_adx_params in order); int32 cus, hook, nch, want_rc; int32 lengths[nch];
//                  when want_rc == 0:
//                  int64 pcm_off[nch], adx_off[nch]; int64 pcm_samples, adx_bytes, total_frames, encode_ws, decode_ws;
//                  int32 order[nch];
//                  twice (encoder, decoder): int32 segments, seg_frames, items; int32 item[2 * items] }
// Every array the header fills is a heap block of exactly its size.  Prints "<layouts> <refused> <items> ok" and exits 0,
// or says what differs and exits 1.
#include "../../vgaudio_amd/csrc/adx_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace {
thread_local char g_error[512];
}

void vga::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

using namespace vga;

namespace {

template <class T> bool read_n(FILE *f, T *out, size_t count) { return count == 0 || fread(out, sizeof(T), count, f) == count; }

int fail(const char *what, int index, long long got, long long want)
{
    printf("%s, case %d: got %lld, want %lld (%s)\n", what, index, got, want, g_error);
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) { printf("usage: adx_host_driver cases.bin\n"); return 2; }
    int n = 0, layouts = 0, refused = 0;
    long long items_seen = 0;
    if (!read_n(f, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int pf[8], head[4];
        if (!read_n(f, pf, 8) || !read_n(f, head, 4)) return 2;
        const int cus = head[0], hook = head[1], nch = head[2], want_rc = head[3];
        vga_adx_params p;
        memset(&p, 0, sizeof p);
        p.sample_rate = pf[0]; p.highpass_frequency = pf[1]; p.frame_size = pf[2]; p.version = pf[3];
        p.history = (int16_t)pf[4]; p.padding = pf[5]; p.type = pf[6]; p.filter = pf[7];
        std::vector<int> lengths(nch > 0 ? nch : 0);
        if (!read_n(f, lengths.data(), lengths.size())) return 2;
        adx::RaggedLayout *L = new adx::RaggedLayout;
        const int rc = adx::make_layout(&p, nch > 0 ? lengths.data() : nullptr, nch, *L);
        if (rc != want_rc) return fail("make_layout", i, rc, want_rc);
        if (rc) {
            refused++;
            delete L;
            continue;
        }
        std::vector<int64_t> pcm_off(nch), adx_off(nch);
        int64_t totals[5];
        std::vector<int> order(nch);
        if (!read_n(f, pcm_off.data(), nch) || !read_n(f, adx_off.data(), nch) || !read_n(f, totals, 5) || !read_n(f, order.data(), nch)) return 2;
        for (int c = 0; c < nch; c++) {
            if (L->pcm_off[c] != pcm_off[c]) return fail("pcm offset", i, L->pcm_off[c], pcm_off[c]);
            if (L->adx_off[c] != adx_off[c]) return fail("adx offset", i, L->adx_off[c], adx_off[c]);
            if (L->order[c] != order[c]) return fail("order", i, L->order[c], order[c]);
        }
        const int64_t got[5] = {L->totals.pcm_samples, L->totals.adx_bytes, L->totals.total_frames,
                                (int64_t)L->totals.encode_workspace_bytes, (int64_t)L->totals.decode_workspace_bytes};
        for (int k = 0; k < 5; k++)
            if (got[k] != totals[k]) return fail("totals", i, got[k], totals[k]);
        if (L->totals.channels != nch) return fail("channels", i, L->totals.channels, nch);
        for (int dir = 0; dir < 2; dir++) {
            int ph[3];
            if (!read_n(f, ph, 3)) return 2;
            std::vector<int> want_items(2 * (size_t)ph[2]);
            if (!read_n(f, want_items.data(), want_items.size())) return 2;
            const adx::RaggedPlan plan = adx::make_plan(*L, cus, hook, dir == 0);
            if (nch > 0 && plan.pieces.segments != ph[0]) return fail(dir ? "decode pieces" : "encode pieces", i, plan.pieces.segments, ph[0]);
            if (nch > 0 && plan.pieces.seg_frames != ph[1]) return fail(dir ? "decode seg_frames" : "encode seg_frames", i, plan.pieces.seg_frames, ph[1]);
            if (plan.item_count() != ph[2]) return fail("items", i, plan.item_count(), ph[2]);
            if (plan.pieces.segments > adx::MAX_PIECES) return fail("more than 64 pieces", i, plan.pieces.segments, adx::MAX_PIECES);
            for (size_t k = 0; k < want_items.size(); k++)
                if (plan.items[k] != want_items[k]) return fail("item table", i, plan.items[k], want_items[k]);
            // what a call cuts its workspace into lies inside what the layout reports
            const size_t used = dir == 0 ? adx::cut_encode_workspace(L->slots(), plan.pieces.segments, L->lane_frames).bytes
                                         : adx::cut_decode_workspace(L->slots(), plan.pieces.segments).bytes;
            const size_t room = dir == 0 ? L->totals.encode_workspace_bytes : L->totals.decode_workspace_bytes;
            if (L->time_pieces && nch > 0 && used > room) return fail("workspace", i, (long long)used, (long long)room);
            items_seen += plan.item_count();
        }
        layouts++;
        delete L;
    }
    fclose(f);
    printf("%d %d %lld ok\n", layouts, refused, items_seen);
    return 0;
}
