// runtime.hip -- the library's own state, shared by every codec's entry points: the error report, the device list, the
// progress callback, the calling thread's test settings and the last pipeline's report (include/vgaudio_hip.h,
// include/vgaudio_hip_testing.h).
#include "common.hpp"
#include "host_batch.hpp"
#include "../../include/vgaudio_hip_testing.h"

namespace vga {

static thread_local char g_err[512] = "";
static thread_local bool g_err_pending = false;

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    g_err_pending = true;
}

bool take_error_pending()
{
    const bool was = g_err_pending;
    g_err_pending = false;
    return was;
}

int require_device()
{
    // every entry point that is going to touch the device passes here first: a failure of an EARLIER call on this thread
    // (an argument check, say) must not make this call's buffers synchronise the device when they are released
    g_err_pending = false;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (%s); libvgaudio_hip has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return VGA_ERR_DEVICE;
    }
    return VGA_OK;
}

// test hooks (include/vgaudio_hip_testing.h): per calling thread, so that no call on another thread is affected
static thread_local ThreadSettings g_settings;
ThreadSettings &thread_settings() { return g_settings; }
int force_open_seams() { return g_settings.force_open_seams; }
int encoder_layout() { return g_settings.encoder_layout; }
int coefs_kernel_variant() { return g_settings.coefs_variant; }
int encoder_segments_override() { return g_settings.encoder_segments; }
int encoder_persistent_mode() { return g_settings.encoder_persistent; }
int hca_frames_per_group_override() { return g_settings.hca_frames_per_group; }
bool gc_seam_handover_off() { return g_settings.gc_seam_handover_off != 0; }
const int *gc_schedule_override() { return g_settings.gc_schedule[0] > 0 ? g_settings.gc_schedule : nullptr; }
// not a setting but a record: what the calling thread's last ADX launches chose (0 = none yet)
static thread_local int g_adx_encode_path = 0, g_adx_decode_path = 0;
void note_adx_encode_path(int path) { g_adx_encode_path = path; }
void note_adx_decode_path(int path) { g_adx_decode_path = path; }

// The host pipeline runs an upload stream, a download stream and two lanes of kernels next to whatever streams the host
// has; the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (the runtime's default of four unless the
// host sets it), and a copy stream that shares a queue with a kernel stream waits behind that stream's kernels (measured:
// every download of a 4096-channel encode ended only when the last kernel had, 660 ms instead of 533 ms).  So the calls run
// a second kernel lane only when the host has configured enough queues for it.  How many hardware queues a process opens
// is the host's decision (the queues of a GPU are shared by every process on it): the library reads the variable and
// never sets it.
static int g_queues_seen_by_runtime = 4;             // what the HIP runtime reads from the variable (its default when unset)
__attribute__((constructor)) static void read_hardware_queues()
{
    if (const char *host = std::getenv("GPU_MAX_HW_QUEUES"))
        g_queues_seen_by_runtime = std::atoi(host);
}
int hardware_queues_requested() { return g_queues_seen_by_runtime; }

static std::mutex g_devices_mutex;
static std::vector<int> g_devices;                   // vga_set_devices(); empty = the caller's current device
std::vector<int> batch_devices()
{
    std::lock_guard<std::mutex> g(g_devices_mutex);
    return g_devices;
}

static thread_local PipeReport g_pipe_report;
PipeReport &pipe_report() { return g_pipe_report; }
static thread_local ProgressCallback g_progress_callback;
ProgressCallback progress_callback() { return g_progress_callback; }
static thread_local ProgressSink *g_progress_sink = nullptr;
ProgressSink *&current_progress_sink() { return g_progress_sink; }

}  // namespace vga

using namespace vga;

extern "C" {

const char *vga_last_error(void) { return g_err; }

const char *vga_version(void) { return "vgaudio_hip 0.2 (gfx950)"; }

void vga_release_cached_memory(void)
{
    DevicePool::get().trim();
    pipe::PinnedPool::get().trim();
    pipe::MaskedStreamPool::get().trim();
}

int vga_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vga_set_device(int device)
{
    VGA_HIP_TRY(hipSetDevice(device));
    return VGA_OK;
}

int vga_set_devices(const int *devices, int count)
{
    if (count < 0 || (count > 0 && !devices) || count > 64) { set_error("vga_set_devices: bad device list"); return VGA_ERR_ARGUMENT; }
    int n = 0;
    if (count > 0 && (hipGetDeviceCount(&n) != hipSuccess || n <= 0)) {
        set_error("no HIP device available; libvgaudio_hip has no CPU fallback");
        return VGA_ERR_DEVICE;
    }
    for (int i = 0; i < count; i++)
        if (devices[i] < 0 || devices[i] >= n) { set_error("vga_set_devices: device %d of %d does not exist", devices[i], n); return VGA_ERR_ARGUMENT; }
    std::lock_guard<std::mutex> g(g_devices_mutex);
    g_devices.assign(devices, devices + count);
    return VGA_OK;
}

int vga_get_devices(int *devices, int capacity)
{
    std::lock_guard<std::mutex> g(g_devices_mutex);
    for (int i = 0; i < (int)g_devices.size() && i < capacity && devices; i++) devices[i] = g_devices[i];
    return (int)g_devices.size();
}

int vga_set_progress_callback(vga_progress_fn fn, void *user)
{
    g_progress_callback.fn = fn;
    g_progress_callback.user = fn ? user : nullptr;
    return VGA_OK;
}

// ---------------------------------------------------------------- test hooks (include/vgaudio_hip_testing.h)
int vga_testing_force_open_seams_this_thread(int mode)
{
    const int old = g_settings.force_open_seams;
    g_settings.force_open_seams = mode;
    return old;
}
int vga_testing_gc_encoder_layout_this_thread(int channels_per_wave)
{
    const int old = g_settings.encoder_layout;
    if (channels_per_wave == 0 || channels_per_wave == 1 || channels_per_wave == 4 || channels_per_wave == 8)
        g_settings.encoder_layout = channels_per_wave;
    return old;
}
int vga_testing_gc_coefs_variant_this_thread(int variant)
{
    const int old = g_settings.coefs_variant;
    if (variant >= 0 && variant <= 3) g_settings.coefs_variant = variant;
    return old;
}
int vga_testing_gc_encoder_segments_this_thread(int segments)
{
    const int old = g_settings.encoder_segments;
    g_settings.encoder_segments = segments > 0 ? segments : 0;
    return old;
}
int vga_testing_gc_encoder_persistent_this_thread(int mode)
{
    const int old = g_settings.encoder_persistent;
    g_settings.encoder_persistent = mode >= 0 && mode <= 2 ? mode : 0;
    return old;
}
int vga_testing_gc_seam_handover_this_thread(int on)
{
    const int old = g_settings.gc_seam_handover_off ? 0 : 1;
    g_settings.gc_seam_handover_off = on ? 0 : 1;
    return old;
}
int vga_testing_gc_schedule_this_thread(int big_rounds, const int *tail_counts, const int *tail_frames, int min_tail_frames)
{
    int *s = g_settings.gc_schedule;
    const int old = s[0];
    for (int i = 0; i < 8; i++) s[i] = 0;
    if (big_rounds <= 0 || !tail_counts || !tail_frames) return old;
    s[0] = big_rounds;
    s[7] = min_tail_frames < 64 ? 64 : min_tail_frames;
    for (int i = 0; i < 3; i++) {
        s[1 + i] = tail_counts[i] > 0 ? tail_counts[i] : 0;
        s[4 + i] = tail_frames[i] < s[7] ? s[7] : tail_frames[i];
    }
    return old;
}
int vga_testing_hca_frames_per_group_this_thread(int frames)
{
    const int old = g_settings.hca_frames_per_group;
    g_settings.hca_frames_per_group = frames > 0 ? frames : 0;
    return old;
}
int vga_testing_adx_last_path_this_thread(int *encode, int *decode)
{
    if (encode) *encode = g_adx_encode_path;
    if (decode) *decode = g_adx_decode_path;
    return 0;
}
void vga_testing_host_pipeline_this_thread(int feeders, int drainers, int chunk_units, int slot_bytes)
{
    PipeOverride &o = g_settings.pipe;
    o.feeders = feeders;
    o.drainers = drainers;
    o.chunk_units = chunk_units;
    o.slot_bytes = slot_bytes;
}
void vga_testing_host_pipeline_tail_this_thread(int tail_units) { g_settings.pipe.tail_units = tail_units > 0 ? tail_units : 0; }
void vga_testing_buckets_order_this_thread(int order) { g_settings.pipe.buckets_order = order == 1 || order == 2 ? order : 0; }
void vga_testing_host_transfer_this_thread(int mode) { g_settings.pipe.transfer = mode == 1 || mode == 2 ? mode : 0; }
void vga_testing_host_transfer_piece_bytes_this_thread(int bytes) { g_settings.pipe.piece_bytes = bytes > 0 ? bytes : 0; }
void vga_testing_fail_step_this_thread(int kind, int nth)
{
    const bool on = kind >= VGA_TESTING_STEP_CHUNK_COMPUTE && kind <= VGA_TESTING_STEP_HCA_STREAM_FRAMES && nth > 0;
    g_settings.fail = FailStep{on ? kind : 0, on ? nth : 0, 0};
}
void vga_testing_host_compute_lanes_this_thread(int lanes) { g_settings.pipe.compute_lanes = lanes > 0 ? lanes : 0; }
int vga_testing_poison_allocations(int byte)
{
    if (byte < -1 || byte > 255) return poison_byte();
    return poison_setting().exchange(byte, std::memory_order_relaxed);
}

int vga_testing_plan_buckets(const int *group, const int *length, int n, int max_units, long long max_volume, int longest_first,
                             int *order_out, int *chunk_begin_out, int *chunk_length_out, int *chunk_group_out, int max_chunks)
{
    if (n < 0 || (n > 0 && (!group || !length))) return -1;
    const BucketPlan plan = plan_buckets(std::vector<int>(group, group + n), std::vector<int>(length, length + n), max_units, max_volume, longest_first != 0);
    const int chunks = (int)plan.chunk_begin.size() - 1;
    if (chunks > max_chunks) return -1;
    for (int i = 0; i < n && order_out; i++) order_out[i] = plan.order[i];
    for (int k = 0; k <= chunks && chunk_begin_out; k++) chunk_begin_out[k] = plan.chunk_begin[k];
    for (int k = 0; k < chunks; k++) {
        if (chunk_length_out) chunk_length_out[k] = plan.chunk_length[k];
        if (chunk_group_out) chunk_group_out[k] = plan.chunk_group[k];
    }
    return chunks;
}
int vga_testing_last_pipeline_stats(double *out, int n)
{
    const PipeReport &r = g_pipe_report;
    const double v[] = {r.stats.total, r.stats.setup, r.stats.feed_copy, r.stats.feed_wait_slot, r.stats.feed_issue, r.stats.feed_max,
                        r.stats.main_wait_upload, r.stats.main_launch, r.stats.main_tail_sync, r.stats.drain_wait_compute,
                        r.stats.drain_wait_copy, r.stats.drain_copy, r.stats.drain_max, (double)r.stats.feeders, (double)r.stats.drainers,
                        (double)r.stats.chunks, (double)r.stats.chunk_units, r.t_alloc, r.t_entry, r.stats.feed_boundary, r.stats.feed_final, r.stats.drain_register};
    const int m = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n && i < m; i++) out[i] = v[i];
    return m;
}

}  // extern "C"
