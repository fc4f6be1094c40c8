// Stand-in (the project's own text, see ref_host.hpp) for the names of <cooperative_groups.h> the reference uses:
// this_grid().thread_rank(), this_thread_block() with group_index / thread_index / thread_rank / sync.
#pragma once
#include "ref_host.hpp"

namespace cooperative_groups {

struct grid_group {
    // blocks in x-fastest order, the block's threads in x-fastest order
    unsigned long long thread_rank() const {
        const ref_host::ThreadPlace& p = ref_host::g_scheduler.place;
        const unsigned long long block = ((unsigned long long)p.block_idx.z * p.grid_dim.y + p.block_idx.y) * p.grid_dim.x + p.block_idx.x;
        const unsigned long long in_block = ((unsigned long long)p.thread_idx.z * p.block_dim.y + p.thread_idx.y) * p.block_dim.x + p.thread_idx.x;
        return block * ((unsigned long long)p.block_dim.x * p.block_dim.y * p.block_dim.z) + in_block;
    }
};

struct thread_block {
    dim3 group_index() const { return ref_host::g_scheduler.place.block_idx; }
    dim3 thread_index() const { return ref_host::g_scheduler.place.thread_idx; }
    unsigned int thread_rank() const {
        const ref_host::ThreadPlace& p = ref_host::g_scheduler.place;
        return (p.thread_idx.z * p.block_dim.y + p.thread_idx.y) * p.block_dim.x + p.thread_idx.x;
    }
    void sync() const { ref_host::barrier(0); }
};

inline grid_group this_grid() { return grid_group(); }
inline thread_block this_thread_block() { return thread_block(); }

}  // namespace cooperative_groups
