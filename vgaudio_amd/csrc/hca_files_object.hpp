// hca_files_object.hpp -- what a vga_hca_files object is (capi_hca_files.hip creates and destroys it), for the C-ABI files
// that serve calls on it: capi_hca_files.hip and capi_hca_keyed_files.hip.  The shared part is files_object.hpp's
// (DESIGN.md 4.6n).
#pragma once
#include "files_object.hpp"
#include "hca_files_kernels.hpp"
#include "hca_keyed_files_host.hpp"

struct vga_hca_files {
    static constexpr const char *type_name = "vga_hca_files";
    vga::hcaf::FilesLayout L;
    vga::hcak::FindTables find;                  // (a set from parsed headers) what the key search needs of every file
    vga::fileset::TableBlock block;
    vga::hcaf::DeviceTables tables;
    int files() const { return L.totals.files; }
};

namespace vga {
namespace hcaf {

extern thread_local int g_force_general;         // vga_hca_files_force_general_this_thread
using fileset::check_object;

}  // namespace hcaf
}  // namespace vga
