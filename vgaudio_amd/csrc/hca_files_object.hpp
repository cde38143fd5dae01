// hca_files_object.hpp -- what a vga_hca_files object is (capi_hca_files.hip creates and destroys it), for the C-ABI files
// that serve calls on it: capi_hca_files.hip and capi_hca_keyed_files.hip.
#pragma once
#include "common.hpp"
#include "hca_files_kernels.hpp"
#include "hca_keyed_files_host.hpp"

struct vga_hca_files {
    vga::hcaf::FilesLayout L;
    vga::hcak::FindTables find;                  // (a set from parsed headers) what the key search needs of every file
    void *d_tables = nullptr;
    vga::hcaf::DeviceTables tables;
    int device = 0;
    ~vga_hca_files()
    {
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace vga {
namespace hcaf {

extern thread_local int g_force_general;         // vga_hca_files_force_general_this_thread
// null object, or made on another device than the current one: VGA_ERR_ARGUMENT, `what` in front of the message
int check_object(const vga_hca_files *s, const char *what);

}  // namespace hcaf
}  // namespace vga
