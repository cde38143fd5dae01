// adx_files_object.hpp -- what a vga_adx_files object is (capi_adx_files.hip creates and destroys it), for the C-ABI files
// that serve calls on it: capi_adx_files.hip and capi_adx_keyed_files.hip.
#pragma once
#include "common.hpp"
#include "adx_files_kernels.hpp"

struct vga_adx_files {
    vga::adxf::FilesLayout L;
    void *d_tables = nullptr;
    vga::adxf::DeviceTables tables;
    int device = 0;
    ~vga_adx_files()
    {
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace vga {
namespace adxf {

extern thread_local int g_force_general;         // vga_adx_files_force_general_this_thread
// null object, or made on another device than the current one: VGA_ERR_ARGUMENT, `what` in front of the message
int check_object(const vga_adx_files *s, const char *what);

}  // namespace adxf
}  // namespace vga
