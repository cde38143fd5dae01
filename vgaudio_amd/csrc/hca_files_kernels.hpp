// hca_files_kernels.hpp -- launchers of hca_files_kernels.hip over the device tables of a vga_hca_files object
#pragma once
#include "common.hpp"
#include "hca_files_host.hpp"
#include "hca_keyed_walk.hpp"

namespace vga {
namespace hcaf {

// the object's tables in device memory (hca_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const uint8_t *headers = nullptr;            // (a set for writing) every header, each at a multiple of 16
    const uint8_t *tables = nullptr;             // the substitution tables, 256 bytes each
    const uint16_t *crc_pow = nullptr;           // vga::hca::crc_pow_table
    const Item *items[2] = {nullptr, nullptr};   // every file in its own form (span items in front); every file general
    int files = 0;
    int span_items = 0, item_count[2] = {0, 0};
    // (a set from parsed headers) for the key search of hca_keyed_files_kernels.hip
    const hcak::WalkFile *walk = nullptr;        // per file
    const int *find_files = nullptr;             // the type-56 files
    int find_file_count = 0, find_max_channels = 1;
};

// Where an item's substitution table comes from.  The default is the object's: FileTab::key into DeviceTables::tables.
// external != 0 (hca_keyed_files.h): the caller's tables in device memory, at any byte, and one index per file read by the
// item (index == nullptr: table 0 for every file); an index outside [0, ntables) moves the file unkeyed.
struct KeySource {
    const uint8_t *tables = nullptr;
    const int *index = nullptr;
    int ntables = 0;
    int external = 0;
};

// general: the force hook's table
int launch_write_images(const DeviceTables &t, bool general, const uint8_t *d_frames, uint8_t *d_images, hipStream_t stream);
int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_frames, int *d_bad_crc, hipStream_t stream,
                       const KeySource &keys = KeySource());

}  // namespace hcaf
}  // namespace vga
