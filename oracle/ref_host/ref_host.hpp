// ref_host.hpp — host stand-ins for what the reference's three CUDA translation units (GSCuda.cu, AuxBuffer.cu,
// CudaHelpers.cu) take from the CUDA runtime and from cooperative_groups, so that plain g++ compiles their own text and
// the result runs on the CPU. TEST INFRASTRUCTURE ONLY (same rules as gsr_oracle.cpp).
//
// All of this is the project's own text; nothing is taken from CUDA's headers. What it provides:
//   - the function-space words (__global__, __device__, ...) as nothing, __shared__ as `static` (one block is in flight
//     at a time, so a function-local static IS the block's shared memory);
//   - dim3, cudaMemcpy / cudaMemset / cudaDeviceSynchronize on host memory, atomicMin;
//   - the float overloads of the unqualified exp / ceil / round / sqrt a device compile resolves to (<math.h> of the C++
//     library declares them in the global namespace; checked by the static_asserts below);
//   - ref_host::launch(grid, block, kernel, args...): what oracle/build_ref.py writes in place of kernel<<<grid, block>>>(args).
//     Blocks run one after the other. The threads of a block are cooperatively scheduled fibers (ucontext): a thread
//     runs until it returns or reaches a barrier; when every live thread of the block has arrived the barrier opens.
//     A fiber whose thread returned takes the block's next unstarted thread itself, so a kernel without barriers runs a
//     whole block on one fiber. Fiber stacks are kept for the next block and the next launch.
// Not thread safe: one launch at a time per process.
#pragma once

#include <math.h>
#include <ucontext.h>

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static

static_assert(std::is_same<decltype(exp(1.0f)), float>::value, "unqualified exp(float) must be the float overload");
static_assert(std::is_same<decltype(ceil(1.0f)), float>::value, "unqualified ceil(float) must be the float overload");
static_assert(std::is_same<decltype(round(1.0f)), float>::value, "unqualified round(float) must be the float overload");
static_assert(std::is_same<decltype(sqrt(1.0f)), float>::value, "unqualified sqrt(float) must be the float overload");

struct dim3 {
    unsigned int x, y, z;
    constexpr dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

enum cudaError_t { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2,
                      cudaMemcpyDeviceToDevice = 3, cudaMemcpyDefault = 4 };

inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t bytes, cudaMemcpyKind) {
    std::memmove(dst, src, bytes);
    return cudaSuccess;
}
inline cudaError_t cudaMemset(void* dst, int value, size_t bytes) {
    std::memset(dst, value, bytes);
    return cudaSuccess;
}
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }

// (threads of a block take turns, so a plain read-modify-write is atomic)
inline unsigned int atomicMin(unsigned int* address, unsigned int value) {
    const unsigned int old = *address;
    if (value < old) *address = value;
    return old;
}

namespace ref_host {

struct ThreadPlace { dim3 grid_dim, block_dim, block_idx, thread_idx; };

struct Fiber {
    ucontext_t context;
    char* stack = nullptr;
    unsigned int thread = 0;      // the thread of the block this fiber is running
    bool parked = false;          // waiting at a barrier
    int predicate = 0, count = 0; // what it brought to the barrier, what the barrier answers
};

struct Scheduler {
    ucontext_t main;
    std::vector<Fiber*> pool;     // stacks live until the process ends
    Fiber* current = nullptr;
    void (*body)(void*) = nullptr;
    void* body_arg = nullptr;
    unsigned int threads = 0, next = 0;
    ThreadPlace place;
};

inline Scheduler g_scheduler;
constexpr size_t kFiberStackBytes = 256 * 1024;

inline void place_thread(unsigned int t) {
    Scheduler& s = g_scheduler;
    s.place.thread_idx.x = t % s.place.block_dim.x;
    s.place.thread_idx.y = (t / s.place.block_dim.x) % s.place.block_dim.y;
    s.place.thread_idx.z = t / (s.place.block_dim.x * s.place.block_dim.y);
}

// A fiber's whole life: take unstarted threads of the block in flight until none is left, hand back, and start over
// when the scheduler resumes it for a later block.
inline void fiber_main() {
    Scheduler& s = g_scheduler;
    for (;;) {
        Fiber* self = s.current;
        while (s.next < s.threads) {
            self->thread = s.next++;
            place_thread(self->thread);
            s.body(s.body_arg);
        }
        swapcontext(&self->context, &s.main);
    }
}

inline void resume(Fiber* f) {
    Scheduler& s = g_scheduler;
    s.current = f;
    swapcontext(&s.main, &f->context);
}

// Every thread of the block that has not returned arrives here; the answer is how many of them brought a non-zero
// predicate (__syncthreads_count; block.sync() ignores it).
inline int barrier(int predicate) {
    Scheduler& s = g_scheduler;
    Fiber* self = s.current;
    self->predicate = predicate;
    self->parked = true;
    swapcontext(&self->context, &s.main);
    return self->count;
}

inline void run_block() {
    Scheduler& s = g_scheduler;
    s.next = 0;
    size_t used = 0;
    while (s.next < s.threads) {
        if (used == s.pool.size()) {
            Fiber* f = new Fiber;
            f->stack = static_cast<char*>(std::malloc(kFiberStackBytes));
            assert(f->stack);
            getcontext(&f->context);
            f->context.uc_stack.ss_sp = f->stack;
            f->context.uc_stack.ss_size = kFiberStackBytes;
            f->context.uc_link = nullptr;
            makecontext(&f->context, fiber_main, 0);
            s.pool.push_back(f);
        }
        Fiber* f = s.pool[used++];
        f->parked = false;
        resume(f);
    }
    for (;;) {
        int waiting = 0, count = 0;
        for (size_t i = 0; i < used; ++i)
            if (s.pool[i]->parked) { ++waiting; count += s.pool[i]->predicate ? 1 : 0; }
        if (!waiting) break;
        for (size_t i = 0; i < used; ++i) {
            Fiber* f = s.pool[i];
            if (!f->parked) continue;
            f->parked = false;
            f->count = count;
            place_thread(f->thread);
            resume(f);              // to its next barrier (parked again: the next round's) or to its thread's end
        }
    }
}

inline void run_grid(dim3 grid, dim3 block, void (*body)(void*), void* arg) {
    Scheduler& s = g_scheduler;
    s.body = body;
    s.body_arg = arg;
    s.place.grid_dim = grid;
    s.place.block_dim = block;
    s.threads = block.x * block.y * block.z;
    for (unsigned int z = 0; z < grid.z; ++z)
        for (unsigned int y = 0; y < grid.y; ++y)
            for (unsigned int x = 0; x < grid.x; ++x) {
                s.place.block_idx = dim3(x, y, z);
                run_block();
            }
}

// kernel<<<grid, block>>>(args...) of the reference's text. The arguments are converted to the kernel's parameter types
// for every thread, as a by-value kernel parameter is.
template <typename... P, typename... A>
void launch(dim3 grid, dim3 block, void (*kernel)(P...), A&&... args) {
    auto call = [&]() { kernel(args...); };
    run_grid(grid, block, [](void* c) { (*static_cast<decltype(call)*>(c))(); }, &call);
}

}  // namespace ref_host

inline int __syncthreads_count(int predicate) { return ref_host::barrier(predicate); }
