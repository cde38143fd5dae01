// adx_files_object.hpp -- what a vga_adx_files object is (capi_adx_files.hip creates and destroys it), for the C-ABI files
// that serve calls on it: capi_adx_files.hip and capi_adx_keyed_files.hip.  The shared part is files_object.hpp's
// (DESIGN.md 4.6n).
#pragma once
#include "files_object.hpp"
#include "adx_files_kernels.hpp"

struct vga_adx_files {
    static constexpr const char *type_name = "vga_adx_files";
    vga::adxf::FilesLayout L;
    vga::fileset::TableBlock block;
    vga::adxf::DeviceTables tables;
    int files() const { return L.totals.files; }
};

namespace vga {
namespace adxf {

extern thread_local int g_force_general;         // vga_adx_files_force_general_this_thread
using fileset::check_object;

}  // namespace adxf
}  // namespace vga
