// dh_pool.cpp -- the two caching allocators of libdentist_hip.so: device blocks in size-class free lists (dh_dev_*) and
// pooled page-locked host memory (dh_pinned_*).  Owns their maps and mutexes; dh_ctx_destroy trims both.
#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>

#include "dh_internal.h"

// ------------------------------------------------------------------------------------ allocator
namespace {
std::mutex g_alloc_mu;
// free blocks per (device, size class): a block is only handed back to the device it lives on
std::map<std::pair<int, size_t>, std::vector<void *>> g_free_lists;
std::unordered_map<void *, std::pair<int, size_t>> g_block_size;
int current_device()
{
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
size_t size_class(size_t bytes)
{
    if (bytes < 4096) return 4096;
    size_t p = 4096;
    while (p < bytes) p <<= 1;  // next power of two, then steps of p/8 below it
    const size_t step = p >> 4;
    return (bytes + step - 1) / step * step;
}
}  // namespace

hipError_t dh_dev_alloc(void **p, size_t bytes)
{
    const size_t cls = size_class(bytes);
    const int dev = current_device();
    {
        std::lock_guard<std::mutex> lk(g_alloc_mu);
        auto it = g_free_lists.find(std::make_pair(dev, cls));
        if (it != g_free_lists.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, cls);
    if (e != hipSuccess) {  // out of memory: drop the cache and retry once
        (void)hipGetLastError();  // (the failure is sticky: a later hipGetLastError() after a launch would report it)
        dh_dev_trim();
        e = hipMalloc(p, cls);
        if (e != hipSuccess) (void)hipGetLastError();
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_alloc_mu);
        g_block_size[*p] = std::make_pair(dev, cls);
    }
    return e;
}

void dh_dev_free(void *p)
{
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    auto it = g_block_size.find(p);
    if (it == g_block_size.end()) {
        (void)hipFree(p);
        return;
    }
    g_free_lists[it->second].push_back(p);
}

void dh_dev_trim()
{
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    for (auto &kv : g_free_lists)
        for (void *p : kv.second) {
            g_block_size.erase(p);
            (void)hipFree(p);
        }
    g_free_lists.clear();
}

// pooled page-locked host memory (power-of-two classes from 64 KiB); smaller requests and the
// no-device case use malloc
namespace {
std::mutex g_pin_mu;
std::map<size_t, std::vector<void *>> g_pin_free;
std::unordered_map<void *, size_t> g_pin_size;  // pinned blocks (in use or pooled) -> class
size_t g_pin_pooled = 0;
constexpr size_t PIN_MIN = 1u << 16, PIN_POOL_MAX = 4ull << 30;
size_t pin_class(size_t bytes)
{
    size_t p = PIN_MIN;
    while (p < bytes) p <<= 1;
    return p;
}
}  // namespace

void *dh_pinned_alloc(size_t bytes)
{
    if (bytes < PIN_MIN) return malloc(std::max<size_t>(bytes, 1));
    const size_t cls = pin_class(bytes);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_free.find(cls);
        if (it != g_pin_free.end() && !it->second.empty()) {
            void *p = it->second.back();
            it->second.pop_back();
            g_pin_pooled -= cls;
            return p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, cls, hipHostMallocDefault) == hipSuccess && p) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        g_pin_size[p] = cls;
        return p;
    }
    (void)hipGetLastError();
    return malloc(bytes);
}

void dh_pinned_free(void *p, size_t bytes)
{
    if (!p) return;
    if (bytes >= PIN_MIN) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_size.find(p);
        if (it != g_pin_size.end()) {
            if (g_pin_pooled + it->second <= PIN_POOL_MAX) {
                g_pin_free[it->second].push_back(p);
                g_pin_pooled += it->second;
            } else {
                g_pin_size.erase(it);
                (void)hipHostFree(p);
            }
            return;
        }
    }
    free(p);
}

void dh_pinned_trim()
{
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto &kv : g_pin_free)
        for (void *p : kv.second) {
            g_pin_size.erase(p);
            (void)hipHostFree(p);
        }
    g_pin_free.clear();
    g_pin_pooled = 0;
}
