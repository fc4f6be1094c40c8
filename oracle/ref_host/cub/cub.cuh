// Stand-in (the project's own text, see ref_host.hpp) for the two CUB entry points the reference calls:
// DeviceScan::InclusiveSum and DeviceRadixSort::SortPairs, both with the null-temp size query. The scan wraps in the
// output's type, as CUB's does; the sort is stable and compares the key bits [begin_bit, end_bit) only, as a radix
// sort over those bits does. The temporary sizes reported are whatever ref_host::temp_sizes() holds (CUB's own are a
// property of its implementation, not of the reference): oracle/ref_capi.cpp exports a setter, so that a test can
// carve the reference's chunks with this project's sizes and compare every offset.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

#include "../ref_host.hpp"

namespace ref_host {
struct TempSizes {
    size_t scan = 1;        // bytes, whatever the item count (a test sets them per case)
    size_t sort = 1;
};
inline TempSizes g_temp_sizes;
}  // namespace ref_host

namespace cub {

struct DeviceScan {
    template <typename In, typename Out>
    static cudaError_t InclusiveSum(void* temp, size_t& temp_bytes, In in, Out out, int items) {
        if (temp == nullptr) {
            temp_bytes = ref_host::g_temp_sizes.scan;
            return cudaSuccess;
        }
        typename std::remove_reference<decltype(out[0])>::type run = 0;
        for (int i = 0; i < items; ++i) { run += in[i]; out[i] = run; }
        return cudaSuccess;
    }
};

struct DeviceRadixSort {
    template <typename Key, typename Value>
    static cudaError_t SortPairs(void* temp, size_t& temp_bytes, const Key* keys_in, Key* keys_out, const Value* values_in,
                                 Value* values_out, int items, int begin_bit = 0, int end_bit = (int)sizeof(Key) * 8) {
        if (temp == nullptr) {
            temp_bytes = ref_host::g_temp_sizes.sort;
            return cudaSuccess;
        }
        const int width = end_bit - begin_bit;
        const Key mask = width >= (int)sizeof(Key) * 8 ? ~Key(0) : (Key)(((Key(1) << width) - 1) << begin_bit);
        std::vector<int> order(items > 0 ? items : 0);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (keys_in[a] & mask) < (keys_in[b] & mask); });
        for (int i = 0; i < items; ++i) { keys_out[i] = keys_in[order[i]]; values_out[i] = values_in[order[i]]; }
        return cudaSuccess;
    }
};

}  // namespace cub
