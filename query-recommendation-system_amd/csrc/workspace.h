// workspace.h -- how an entry point lays out its caller-allocated workspace, and the host checks around it.
//
// One layout function per workspace: `static FooWs foo_layout(QrCarve &c, sizes...)` takes the regions in order.  The size
// export runs it over a counting carve (QrCarve(nullptr)) and returns bytes(); the entry point and its fill partner run it
// over the caller's pointer.  Nothing else adds up region sizes or walks the workspace, so a size and a carve cannot
// drift apart.  A region advances the carve by its bytes rounded up to `align` (16 unless said): layouts that historically
// round to 256, or not at all (align = 1), say so in the take.  Arrays that one memset or one kernel covers together are
// ONE take, split inside the layout function ("adjacent layout").
#pragma once
#include <stddef.h>
#include <stdint.h>

struct QrCarve {  // base == nullptr: only counts
  explicit QrCarve(const void *ws) : base_(reinterpret_cast<uintptr_t>(ws)) {}
  void *take_bytes(size_t bytes, size_t align = 16) {
    const size_t at = off_;
    off_ += (bytes + align - 1) / align * align;
    return base_ ? reinterpret_cast<void *>(base_ + at) : nullptr;
  }
  // nullptr when counting
  template <typename T> T *take(size_t count, size_t align = 16) {
    return static_cast<T *>(take_bytes(count * sizeof(T), align));
  }
  size_t bytes() const { return off_; }

 private:
  uintptr_t base_;
  size_t off_ = 0;
};

// what `layout(carve, sizes...)` takes: the body of a size export, under its argument guards
#define QR_LAYOUT_BYTES(layout, ...)  \
  ([&] {                              \
    QrCarve c__(nullptr);             \
    layout(c__, __VA_ARGS__);         \
    return c__.bytes();               \
  }())

// array `index` elements into a block that was taken as one (arrays that must stay adjacent); nullptr when counting
template <typename T> static inline T *qr_within(T *block, size_t index) { return block ? block + index : nullptr; }

static inline uintptr_t qr_addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// the workspace holds `need` bytes (QRLSH_EWORKSPACE otherwise); a null workspace holds none
#define QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, need)                                   \
  do {                                                                                              \
    const size_t need__ = (need), got__ = (workspace) ? (size_t)(workspace_bytes) : 0;              \
    if (got__ < need__) {                                                                           \
      qrlsh_set_error("%s: workspace of %zu bytes needed, %zu given", who, need__, got__);          \
      return QRLSH_EWORKSPACE;                                                                      \
    }                                                                                               \
  } while (0)

// `addr` (a qr_addr, or several ORed) is a multiple of `align` bytes (QRLSH_EINVAL otherwise); `what` names the pointers
#define QR_CHECK_ALIGNED(who, what, addr, align) \
  QR_CHECK_ARG((addr) % (align) == 0, "%s: alignment: %s must be %d-byte aligned", who, what, (int)(align))

#define QR_HIP_ASYNC__(who, call, failed)    \
  do {                                       \
    if ((call) != hipSuccess) {              \
      qrlsh_set_error("%s: %s", who, failed); \
      return QRLSH_EHIP;                     \
    }                                        \
  } while (0)
#define QR_MEMSET(who, ptr, value, bytes, st) \
  QR_HIP_ASYNC__(who, hipMemsetAsync(ptr, value, bytes, st), "hipMemsetAsync failed")
// device-to-device copy
#define QR_MEMCPY(who, dst, src, bytes, st) \
  QR_HIP_ASYNC__(who, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync failed")
