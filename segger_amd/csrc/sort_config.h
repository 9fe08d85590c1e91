// The radix sort configuration of the units that sort 64-bit keys (a header of its own: post_common.h stays free of
// rocprim for the units that do not sort).
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

namespace segger {

// rocprim's default onesweep pass for (uint64, int32) pairs on gfx950 ranks with the `match` algorithm and keeps 80 bytes
// of scratch per lane; the `basic` ranking at the same 8 bits per pass and 256 x 12 keys per block compiles without any.
// The same holds for a keys-only sort of uint64.
using NoScratchSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 12>, 8,
                                        rocprim::block_radix_rank_algorithm::basic>>;

}  // namespace segger
