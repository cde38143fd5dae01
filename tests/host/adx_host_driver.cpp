// adx_host_driver.cpp -- vgaudio_amd/csrc/adx_host.hpp on its own (tests/test_adx_ragged_device_host.py,
// tests/test_adx_host_layer.py): the header with a set_error of this file's, no HIP and no product library.  Built twice with g++:
//   * a shared library whose extern "C" wrappers (ah_*) the Python tests compare with the product library's entry points, the
//     oracle's and what the parent answered;
//   * with AddressSanitizer and UBSan, a program that runs a file of cases a test wrote.
// `adx_host_driver cases.bin` -- the ragged layout and plan against the test's own model:
//   int32 n; n x { int32 params[8] (the fields of vga_adx_params in order); int32 cus, hook, nch, want_rc; int32 lengths[nch];
//                  when want_rc == 0:
//                  int64 pcm_off[nch], adx_off[nch]; int64 pcm_samples, adx_bytes, total_frames, encode_ws, decode_ws;
//                  int32 order[nch];
//                  twice (encoder, decoder): int32 segments, seg_frames, items; int32 item[2 * items] }
// Every array the header fills is a heap block of exactly its size.  Prints "<layouts> <refused> <items> ok" and exits 0,
// or says what differs and exits 1.
// `adx_host_driver --calls calls.bin` -- the checks, sizes, conversions and coefficients against recorded answers:
//   int32 n; n x { int32 function (the order of CALLS below); int32 want; int32 message length, message bytes (compared
//                  unless empty); int32 nargs; nargs x { int32 kind; kind 0: int64 value (an int, a dummy address, 0 = null);
//                  kind 1: int32 count, int64 rows[count]; kind 2: int32 count, int32 ints[count];
//                  kind 3: int32 count, count x int32 params[8] } }
// Every array is a heap block of exactly its size: a check that reads row nch ends the run.  Prints "<calls> ok".
#include "../../vgaudio_amd/csrc/adx_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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

// ---- the header's functions for the Python tests.  The eight entry points as the C-ABI files chain the checks, up to the
// device: VGA_OK = every check passed (or there is nothing to do)
extern "C" {

const char *ah_last_error() { return g_error; }

int ah_calculate_coefficients(int highpass_freq, int sample_rate, int16_t *coefs_out)
{
    if (!coefs_out || sample_rate <= 0) { set_error("bad arguments"); return VGA_ERR_ARGUMENT; }
    adx::calculate_coefficients(highpass_freq, sample_rate, coefs_out);
    return VGA_OK;
}
int ah_encoded_byte_count(int pcm_length, const vga_adx_params *p)
{
    return adx::validate(p) != VGA_OK || pcm_length < 0 ? VGA_ERR_ARGUMENT : adx::encoded_byte_count(pcm_length, *p);
}
int ah_encode_device(const int16_t *, int64_t pcm_pitch, int nch, int pcm_length, const vga_adx_params *p, uint8_t *d_out,
                     int64_t out_pitch, int16_t *, void *)
{
    if (int rc = adx::check_encode(p, nch, pcm_length)) return rc;
    if (nch == 0) return VGA_OK;
    return adx::check_encode_device_layout(pcm_pitch, pcm_length, d_out, out_pitch, adx::encoded_byte_count(pcm_length, *p));
}
int ah_decode_device(const uint8_t *, int64_t in_pitch, int adpcm_length, int nch, int sample_count, const vga_adx_params *p, int16_t *,
                     int64_t pcm_pitch, int *, void *)
{
    return adx::check_decode(p, adpcm_length, nch, sample_count, in_pitch, pcm_pitch);
}
int ah_encode_batch(const int16_t *const *pcm, int nch, int pcm_length, const vga_adx_params *p, uint8_t *const *out, int16_t *)
{
    return adx::check_encode(p, nch, pcm_length, true, pcm, out);
}
int ah_decode_batch(const uint8_t *const *adpcm, int adpcm_length, int nch, int sample_count, const vga_adx_params *p, int16_t *const *pcm_out)
{
    return adx::check_decode(p, adpcm_length, nch, sample_count, adpcm_length, sample_count, true, adpcm, pcm_out);
}
int ah_encode_batch_v(const int16_t *const *pcm, const int *lengths, int nch, const vga_adx_params *params, uint8_t *const *out, int16_t *)
{
    return adx::check_encode_v(pcm, lengths, nch, params, out);
}
int ah_decode_batch_v(const uint8_t *const *adpcm, const int *adpcm_lengths, int nch, const int *sample_counts, const vga_adx_params *params,
                      int16_t *const *pcm_out)
{
    return adx::check_decode_v(adpcm, adpcm_lengths, nch, sample_counts, params, pcm_out);
}

int ah_nibble_count_to_sample_count(int n, int frame_size) { return adx::nibble_count_to_sample_count(n, frame_size); }
int ah_sample_count_to_nibble_count(int n, int frame_size) { return adx::sample_count_to_nibble_count(n, frame_size); }
int ah_sample_count_to_byte_count(int n, int frame_size) { return adx::sample_count_to_byte_count(n, frame_size); }
int ah_divide_by_round_up(int v, int d) { return adx::divide_by_round_up(v, d); }
long long ah_encoded_bytes(int pcm_length, const vga_adx_params *p) { return adx::encoded_bytes(pcm_length, *p); }
long long ah_decode_bytes_read(int sample_count, const vga_adx_params *p) { return adx::decode_bytes_read(sample_count, *p); }
int ah_own_frames(int pcm_length, const vga_adx_params *p) { return adx::own_frames(pcm_length, *p); }
// the two coefficients of the kernels' parameters as one int: coef0's 16 bits below coef1's
int ah_device_coefs(const vga_adx_params *p, int encode)
{
    const adx::AdxDeviceParams d = adx::make_device_params(p, encode != 0);
    const int same = d.frame_size == p->frame_size && d.version == p->version && d.type == p->type && d.filter == p->filter &&
                     d.padding == p->padding && d.history == p->history;
    return same ? (int)((uint32_t)(uint16_t)d.coef0 | ((uint32_t)(uint16_t)d.coef1 << 16)) : -1;
}
// ENCODE_* and DECODE_* in the header's order, then PIECE_ALIGN_FRAMES and OWN_FRAME_SAMPLES
void ah_figures(int *out8)
{
    const int v[8] = {adx::ENCODE_WAVES_PER_SIMD, adx::ENCODE_MIN_PIECE_FRAMES, adx::ENCODE_HOOK_FLOOR, adx::DECODE_WAVES_PER_SIMD,
                      adx::DECODE_MIN_PIECE_FRAMES, adx::DECODE_HOOK_FLOOR, adx::PIECE_ALIGN_FRAMES, adx::OWN_FRAME_SAMPLES};
    memcpy(out8, v, sizeof v);
}

}  // extern "C"

namespace {

template <class T> bool read_n(FILE *f, T *out, size_t count) { return count == 0 || fread(out, sizeof(T), count, f) == count; }

int fail(const char *what, int index, long long got, long long want)
{
    printf("%s, case %d: got %lld, want %lld (%s)\n", what, index, got, want, g_error);
    return 1;
}


// ---- --calls: one argument of a recorded call; an array is a heap block of exactly its size
struct Arg {
    long long value = 0;
    void *block = nullptr;
    template <class T> T *as() const { return static_cast<T *>(block); }
};

bool read_arg(FILE *f, Arg &a)
{
    int kind = 0, count = 0;
    if (!read_n(f, &kind, 1)) return false;
    if (kind == 0) return read_n(f, &a.value, 1);
    if (!read_n(f, &count, 1) || count < 0) return false;
    if (kind == 1) {
        a.block = malloc(count * sizeof(void *));
        return read_n(f, a.as<long long>(), count);
    }
    if (kind == 2) {
        a.block = malloc(count * sizeof(int));
        return read_n(f, a.as<int>(), count);
    }
    vga_adx_params *p = static_cast<vga_adx_params *>(malloc(count * sizeof(vga_adx_params)));
    a.block = p;
    for (int i = 0; i < count; i++) {
        int pf[8];
        if (!read_n(f, pf, 8)) return false;
        memset(&p[i], 0, sizeof p[i]);
        p[i].sample_rate = pf[0]; p[i].highpass_frequency = pf[1]; p[i].frame_size = pf[2]; p[i].version = pf[3];
        p[i].history = (int16_t)pf[4]; p[i].padding = pf[5]; p[i].type = pf[6]; p[i].filter = pf[7];
    }
    return true;
}

// an argument as a pointer: its array, or its value as a dummy address
template <class T> T *ptr(const Arg &a) { return a.block ? a.as<T>() : reinterpret_cast<T *>((uintptr_t)a.value); }

enum { CALL_SIZE, CALL_COEFS, CALL_ENCODE_DEVICE, CALL_DECODE_DEVICE, CALL_ENCODE_BATCH, CALL_DECODE_BATCH, CALL_ENCODE_V, CALL_DECODE_V,
       CALL_NIBBLES_TO_SAMPLES, CALL_SAMPLES_TO_NIBBLES, CALL_SAMPLES_TO_BYTES, CALL_CEIL, CALL_DEVICE_COEFS, CALLS };
const int CALL_ARGS[CALLS] = {2, 3, 9, 10, 6, 6, 6, 6, 2, 2, 2, 2, 2};

int run_call(int fn, const Arg *a)
{
    typedef const int16_t *const *pcm_rows;
    typedef const uint8_t *const *byte_rows;
    const int i0 = (int)a[0].value, i1 = (int)a[1].value, i2 = (int)a[2].value, i3 = (int)a[3].value;
    switch (fn) {
    case CALL_SIZE: return ah_encoded_byte_count(i0, ptr<vga_adx_params>(a[1]));
    case CALL_COEFS: {
        int16_t *c = a[2].value ? new int16_t[2] : nullptr;
        const int rc = ah_calculate_coefficients(i0, i1, c);
        delete[] c;
        return rc;
    }
    case CALL_ENCODE_DEVICE:
        return ah_encode_device(ptr<int16_t>(a[0]), a[1].value, i2, i3, ptr<vga_adx_params>(a[4]), ptr<uint8_t>(a[5]), a[6].value, nullptr, nullptr);
    case CALL_DECODE_DEVICE:
        return ah_decode_device(ptr<uint8_t>(a[0]), a[1].value, i2, i3, (int)a[4].value, ptr<vga_adx_params>(a[5]), ptr<int16_t>(a[6]), a[7].value,
                                nullptr, nullptr);
    case CALL_ENCODE_BATCH: return ah_encode_batch((pcm_rows)ptr<void *>(a[0]), i1, i2, ptr<vga_adx_params>(a[3]), (uint8_t *const *)ptr<void *>(a[4]), nullptr);
    case CALL_DECODE_BATCH: return ah_decode_batch((byte_rows)ptr<void *>(a[0]), i1, i2, i3, ptr<vga_adx_params>(a[4]), (int16_t *const *)ptr<void *>(a[5]));
    case CALL_ENCODE_V:
        return ah_encode_batch_v((pcm_rows)ptr<void *>(a[0]), ptr<int>(a[1]), i2, ptr<vga_adx_params>(a[3]), (uint8_t *const *)ptr<void *>(a[4]), nullptr);
    case CALL_DECODE_V:
        return ah_decode_batch_v((byte_rows)ptr<void *>(a[0]), ptr<int>(a[1]), i2, ptr<int>(a[3]), ptr<vga_adx_params>(a[4]),
                                 (int16_t *const *)ptr<void *>(a[5]));
    case CALL_NIBBLES_TO_SAMPLES: return adx::nibble_count_to_sample_count(i0, i1);
    case CALL_SAMPLES_TO_NIBBLES: return adx::sample_count_to_nibble_count(i0, i1);
    case CALL_SAMPLES_TO_BYTES: return adx::sample_count_to_byte_count(i0, i1);
    case CALL_CEIL: return adx::divide_by_round_up(i0, i1);
    default: return ah_device_coefs(ptr<vga_adx_params>(a[0]), i1);
    }
}

int run_calls(FILE *f)
{
    int n = 0;
    if (!read_n(f, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int head[3], nargs = 0;
        if (!read_n(f, head, 3) || head[0] < 0 || head[0] >= CALLS || head[2] < 0) return 2;
        std::string want_message((size_t)head[2], ' ');
        if (!read_n(f, &want_message[0], want_message.size()) || !read_n(f, &nargs, 1) || nargs != CALL_ARGS[head[0]]) return 2;
        Arg args[10];                                                   // (the most a call takes)
        for (int k = 0; k < nargs; k++)
            if (!read_arg(f, args[k])) return 2;
        (void)ah_calculate_coefficients(0, 0, nullptr);                 // the message before the call, as the test left it
        const int got = run_call(head[0], args);
        for (int k = 0; k < nargs; k++) free(args[k].block);
        if (got != head[1]) return fail("call", i, got, head[1]);
        if (!want_message.empty() && want_message != g_error) {
            printf("call %d: message '%s', want '%s'\n", i, g_error, want_message.c_str());
            return 1;
        }
    }
    printf("%d ok\n", n);
    return 0;
}
}  // namespace

int main(int argc, char **argv)
{
    const bool calls = argc > 2 && strcmp(argv[1], "--calls") == 0;
    FILE *f = argc > 1 ? fopen(argv[calls ? 2 : 1], "rb") : nullptr;
    if (!f) { printf("usage: adx_host_driver cases.bin | --calls calls.bin\n"); return 2; }
    if (calls) {
        const int rc = run_calls(f);
        fclose(f);
        return rc;
    }
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
