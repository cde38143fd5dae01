// container_math.hpp -- the reference's small helpers the container layouts share (Helpers.cs, Extensions.cs,
// AudioFormatBaseBuilder.WithLoop) and the two refusals that carry a plain message.  Free of <hip/hip_runtime.h>: the layouts
// that stand-alone host programs include (nw_host.hpp) use them as container_host.hpp does.
#pragma once
#include "gc_host.hpp"
#include "../../include/vgaudio_hip_pcm.h"

namespace vga {
namespace container {

inline int invalid(const char *msg) { set_error("%s", msg); return VGA_ERR_INVALID_DATA; }
inline int out_of_range(const char *msg) { set_error("%s", msg); return VGA_ERR_OUT_OF_RANGE; }

inline int64_t next_multiple(int64_t v, int64_t m) { return m <= 0 || v % m == 0 ? v : v + m - v % m; }   // Helpers.cs:71-80
// Extensions.cs:145, (int)Math.Ceiling((double)v / d): a negative quotient rounds towards zero (-1 / 8 -> 0)
inline int div_round_up(int v, int d) { return v / d + (v % d != 0 && (v < 0) == (d < 0) ? 1 : 0); }
inline int bytes_of(int samples) { return gc::sample_count_to_byte_count(samples); }

// the kind of pitched planar rows a PCM call takes or gives (vgaudio_hip_pcm.h)
inline int check_sample_kind(int kind)
{
    if (kind == VGA_SAMPLES_S16 || kind == VGA_SAMPLES_8BIT) return VGA_OK;
    set_error("unknown sample kind %d", kind);
    return VGA_ERR_ARGUMENT;
}

// AudioFormatBaseBuilder.WithLoop (:30-43)
inline int check_loop(int looping, int loop_start, int loop_end, int sample_count)
{
    if (sample_count < 0) return out_of_range("negative sample count");
    if (!looping) return VGA_OK;
    if (loop_start < 0 || loop_start > sample_count || loop_end < 0 || loop_end > sample_count)
        return out_of_range("Loop points must be less than the number of samples and non-negative.");
    if (loop_end < loop_start) return out_of_range("The loop end must be greater than the loop start");
    return VGA_OK;
}

}  // namespace container
}  // namespace vga
