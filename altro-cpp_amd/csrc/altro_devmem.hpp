// altro_devmem.hpp — who owns the engine's device memory, and how a host caller's arrays (doubles, ints, bytes, statistics
// structs: each copied with its own element count) get to the device and back.
// Host code only: the HIP API header, the standard library and Parts (altro_common.hpp).  The one place of the solver library
// that calls hipMalloc / hipFree / hipHostMalloc / hipHostFree: every block is held by an owner whose destructor frees it.
// Whoever lets a block go while a copy on the engine's stream may still touch it waits for that stream first (Staged does).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "altro_common.hpp"

namespace altro_hip {

struct DeviceMem {
  static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void put(void* p) { (void)hipFree(p); }
};
struct PinnedMem {  // host memory the device sees too (hipHostGetDevicePointer): mapped, coherent
  static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static void put(void* p) { (void)hipHostFree(p); }
};
// One block, freed when its owner goes: one pointer, one size, no pooling.  Move-only.
template <class U, class Mem = DeviceMem>
class DevBlock {
 public:
  DevBlock() = default;
  DevBlock(DevBlock&& o) noexcept : p_(o.p_), count_(o.count_) { o.p_ = nullptr, o.count_ = 0; }
  DevBlock& operator=(DevBlock&& o) noexcept {  // (what this block held goes with `o`)
    std::swap(p_, o.p_);
    std::swap(count_, o.count_);
    return *this;
  }
  ~DevBlock() { reset(); }
  // `count` elements (at least one is asked for), in place of whatever the block held
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = Mem::get((void**)&p_, std::max<size_t>(count, 1) * sizeof(U));
    if (e != hipSuccess) (void)hipGetLastError(), p_ = nullptr;
    count_ = p_ ? count : 0;
    return e;
  }
  void reset() {
    if (p_) Mem::put((void*)p_);
    p_ = nullptr;
    count_ = 0;
  }
  U* get() const { return p_; }
  size_t count() const { return count_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  U* p_ = nullptr;
  size_t count_ = 0;
};
template <class U>
using PinnedBlock = DevBlock<U, PinnedMem>;

// The blocks that live as long as one problem upload: alloc() hands out a raw pointer and keeps the block; all of them go
// when the pool goes (or is assigned a fresh one).  Move-only.
class DevPool {
 public:
  // `count` elements of U (at least one is asked for); *p is null after a failure
  template <class U>
  hipError_t alloc(U** p, size_t count) {
    DevBlock<unsigned char> b;
    const hipError_t e = b.alloc(std::max<size_t>(count, 1) * sizeof(U));
    *p = reinterpret_cast<U*>(b.get());
    if (e == hipSuccess) blocks_.push_back(std::move(b));
    return e;
  }

 private:
  std::vector<DevBlock<unsigned char>> blocks_;
};

// One host call's arrays in ONE device block carved by a Parts<K> layout.  The block and its parts are counted in doubles;
// what a part holds may be doubles, ints, bytes or statistics structs (a layout sizes such a part with DoublesFor<V>), and
// in() / out() copy the caller's elements to the byte, straight from and into the caller's arrays.  in() enqueues the upload
// of a present input part on the stream and out() books the download of a present output part; both hand back what the
// launch is given for that part -- null for an array the caller left out.  part() is for what no caller brings: scratch
// that lives in the block for a direct caller too.  After the caller's launches, finish() enqueues the booked downloads and
// ALWAYS waits for the stream, also after a failure (the block must not go under a copy in flight), and reports the first
// error.  A Staged that goes without finish() while it has uploads on the stream waits for it too.
// `direct`: the caller's arrays are device memory already; they are handed back as they came and nothing is copied.
template <int K>
class Staged {
 public:
  Staged(bool direct, double* block, const Parts<K>& p, hipStream_t stream) : direct_(direct), blk_(block), p_(p), s_(stream) {}
  Staged(const Staged&) = delete;
  ~Staged() { (void)(!done_ && copies_ > 0 && hipStreamSynchronize(s_) != hipSuccess); }
  // part i on the device (a staged block only; null for a part that takes no room)
  double* part(int i) const { return p_.cnt[i] ? blk_ + p_.off[i] : nullptr; }
  // input part i: `count` elements of V from the host array, put at element `first` of the part (two host arrays that share
  // a part: first, then count, as ever).  Exactly count * sizeof(V) bytes go up.  Null, and nothing copied, for a part that
  // cannot hold them.
  template <class V>
  const V* in(int i, const V* host, size_t first, size_t count) {
    if (direct_ || !host) return host;
    if (!p_.cnt[i] || (first + count) * sizeof(V) > p_.cnt[i] * sizeof(double)) return nullptr;
    V* const dev = reinterpret_cast<V*>(blk_ + p_.off[i]) + first;
    if (e_ == hipSuccess) e_ = hipMemcpyAsync(dev, host, count * sizeof(V), hipMemcpyHostToDevice, s_), ++copies_;
    return dev;
  }
  // output part i: exactly `count` elements of V come back into the host array, never a byte past host + count
  template <class V>
  V* out(int i, V* host, size_t count) {
    if (direct_ || !host) return host;
    if (!p_.cnt[i] || count * sizeof(V) > p_.cnt[i] * sizeof(double)) return nullptr;
    V* const dev = reinterpret_cast<V*>(blk_ + p_.off[i]);
    down_[ndown_++] = Down{host, dev, count * sizeof(V)};
    return dev;
  }
  // the whole part, for a V that fills it to the byte: double, or a struct that is a whole number of doubles
  template <class V>
  const V* in(int i, const V* host) {
    static_assert(sizeof(V) % sizeof(double) == 0, "ints and bytes are staged with their count");
    return in(i, host, 0, p_.cnt[i] * sizeof(double) / sizeof(V));
  }
  template <class V>
  V* out(int i, V* host) {
    static_assert(sizeof(V) % sizeof(double) == 0, "ints and bytes are staged with their count");
    return out(i, host, p_.cnt[i] * sizeof(double) / sizeof(V));
  }
  bool ok() const { return e_ == hipSuccess; }
  int copies() const { return copies_; }  // uploads enqueued so far (a caller that launches nothing need not wait without any)
  // `launched`: the caller's launches went out (a launch that was refused leaves nothing to download)
  hipError_t finish(bool launched = true) {
    if (launched && e_ == hipSuccess) e_ = hipGetLastError();
    for (int i = 0; launched && i < ndown_; ++i)
      if (e_ == hipSuccess) e_ = hipMemcpyAsync(down_[i].host, down_[i].dev, down_[i].bytes, hipMemcpyDeviceToHost, s_);
    const hipError_t es = hipStreamSynchronize(s_);
    done_ = true;
    return e_ != hipSuccess ? e_ : es;
  }

 private:
  struct Down { void* host; const void* dev; size_t bytes; };
  const bool direct_;
  double* const blk_;
  const Parts<K> p_;
  const hipStream_t s_;
  Down down_[K] = {};
  int ndown_ = 0, copies_ = 0;
  hipError_t e_ = hipSuccess;
  bool done_ = false;
};

}  // namespace altro_hip
