// poison.hpp -- the test hook vga_testing_poison_allocations (include/vgaudio_hip_testing.h): host state only, shared by
// every allocator of the library (DevicePool, AsyncBuf and device_malloc in common.hpp, PinnedPool in host_pipeline.hpp).
// No HIP here: host_pipeline.hpp is also compiled against the CPU suite's mock runtime.
#pragma once
#include <atomic>

namespace vga {

// -1 (the default): off; 0..255: every block the library allocates is filled with that byte before it is handed out
inline std::atomic<int> &poison_setting()
{
    static std::atomic<int> v{-1};
    return v;
}
// what an allocation pays with the mode off: one relaxed load
inline int poison_byte() { return poison_setting().load(std::memory_order_relaxed); }

}  // namespace vga
