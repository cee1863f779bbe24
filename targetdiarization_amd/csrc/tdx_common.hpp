// tdx_common.hpp — status/error plumbing, the TDXW weight-blob reader, the weight loader (Loader) and the owner of a device
// allocation (DevBuf) shared by the C-ABI translation units.  No exception crosses the C boundary: entry points return a
// TDX_E_* code and leave a message in a thread-local string (include/tdx.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace tdx {

inline std::string& last_error() {
    static thread_local std::string e;
    return e;
}
inline int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}
inline int fail_hip(hipError_t e, const char* file, int line) {
    last_error() = std::string("HIP error: ") + hipGetErrorString(e) + " at " + file + ":" + std::to_string(line);
    return 3;  // TDX_E_HIP
}

inline size_t al(size_t n) { return (n + 63) / 64 * 64; }      // weight images and workspaces are laid out in 64-float units
inline int up(int n, int m) { return (n + m - 1) / m * m; }

// after a kernel launch, inside a function that returns a TDX status
#define LAUNCH_CHECK()                                    \
    do {                                                  \
        hipError_t e__ = hipGetLastError();               \
        if (e__ != hipSuccess) return tdx::fail_hip(e__, __FILE__, __LINE__); \
    } while (0)
#define TRY(x) do { int rc__ = (x); if (rc__ != 0) return rc__; } while (0)

// Makes `device` current for the lifetime of the guard and restores the caller's device afterwards (the
// C-ABI never leaves the calling thread on another device; a forward on a handle whose device is not current
// launches on the handle's device — the stream the caller passes must belong to it).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
        else prev = -1;                 // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct BlobTensor {
    const float* data;
    size_t numel;
    int ndim;
    uint32_t dims[8];
    mutable bool used = false;
};

// TDXW container (targetdiarization_amd/weights.py:pack_blob):
//   "TDXW0001" | u32 n | n x { u16 name_len | name | u8 ndim | u32 dims[ndim] | u64 offset }
//   | zero pad to 64 | data section (f32 little-endian, each tensor 64-byte aligned)
// The header is untrusted input: every count, product and offset is checked without wrap-around.
struct Blob {
    std::map<std::string, BlobTensor> t;
    bool parse(const void* p, size_t bytes) {
        const uint8_t* b = (const uint8_t*)p;
        if (!b || bytes < 12 || memcmp(b, "TDXW0001", 8) != 0) return false;
        size_t pos = 8;
        uint32_t n;
        memcpy(&n, b + pos, 4); pos += 4;
        if ((size_t)n > (bytes - pos) / 11) return false;            // an entry is at least 2 + 0 + 1 + 0 + 8 bytes
        struct Ent { std::string name; BlobTensor bt; uint64_t off; };
        std::vector<Ent> ents;
        ents.reserve(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (bytes - pos < 2) return false;
            uint16_t nl;
            memcpy(&nl, b + pos, 2); pos += 2;
            if (bytes - pos < (size_t)nl + 1) return false;
            Ent e;
            e.name.assign((const char*)b + pos, nl); pos += nl;
            e.bt.ndim = b[pos]; pos += 1;
            if (e.bt.ndim > 8 || bytes - pos < 4u * (size_t)e.bt.ndim + 8) return false;
            uint64_t numel = 1;
            for (int d = 0; d < e.bt.ndim; ++d) {
                memcpy(&e.bt.dims[d], b + pos, 4); pos += 4;
                if (e.bt.dims[d] != 0 && numel > (uint64_t)bytes / e.bt.dims[d]) return false;   // numel*4 could not fit anyway
                numel *= e.bt.dims[d];
            }
            e.bt.numel = (size_t)numel;
            memcpy(&e.off, b + pos, 8); pos += 8;
            ents.push_back(e);
        }
        if (bytes - pos < (64 - pos % 64) % 64) return false;
        const size_t data0 = (pos + 63) / 64 * 64;
        const size_t room = bytes - data0;
        for (auto& e : ents) {
            if (e.off % 4 != 0 || e.off > room) return false;
            if (e.bt.numel > (room - (size_t)e.off) / 4) return false;
            e.bt.data = (const float*)(b + data0 + e.off);
            if (t.count(e.name)) return false;                       // duplicate name
            t[e.name] = e.bt;
        }
        return true;
    }
    const BlobTensor* find(const std::string& name) const {
        auto it = t.find(name);
        if (it == t.end()) return nullptr;
        it->second.used = true;
        return &it->second;
    }
    // first tensor no find() asked for ("" if none): strict loaders reject unexpected keys like
    // load_state_dict(strict=True) does (base_model.py:63)
    std::string first_unused() const {
        for (const auto& kv : t) if (!kv.second.used) return kv.first;
        return std::string();
    }
};

// One hipMalloc allocation, freed with its owner (move-only).  A handle struct holds its weight images as DevBuf members, so
// `delete h` releases them on every path; it reads as the float image it owns (`h->dev + offset`).
class DevBuf {
    void* p_ = nullptr;
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    hipError_t alloc(size_t bytes) {
        if (p_) { (void)hipFree(p_); p_ = nullptr; }
        return hipMalloc(&p_, bytes);
    }
    hipError_t upload(const void* host, size_t bytes) {        // alloc + blocking copy
        const hipError_t e = alloc(bytes);
        return e != hipSuccess ? e : hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice);
    }
    void* get() const { return p_; }
    operator float*() const { return static_cast<float*>(p_); }
};

// What every tdx_*_create does with its blob: look tensors up by name (and size or shape), stage them — as they are, padded,
// or transposed — into one host image at 64-float aligned offsets, then upload the image.  The first tensor that is missing
// or of the wrong size is remembered and reported by finish(); until then get() returns nullptr for it and the push
// functions leave zeros in its place, so a create reads as the list of tensors the model needs.
struct Loader {
    Blob blob;
    std::vector<float> host;
    bool parse(const void* p, size_t bytes) { return blob.parse(p, bytes); }
    bool ok() const { return missing_.empty(); }
    const std::string& missing() const { return missing_; }

    const float* get(const std::string& name, size_t numel) {
        const BlobTensor* t = blob.find(name);
        if (!t || t->numel != numel) return miss(name, false);
        return t->data;
    }
    // name AND shape: a transposed matrix has the right numel and must not load
    const float* get(const std::string& name, std::initializer_list<uint32_t> dims) {
        const BlobTensor* t = blob.find(name);
        bool same = t && t->ndim == (int)dims.size();
        if (same) { int d = 0; for (uint32_t v : dims) same = same && t->dims[d++] == v; }
        if (!same) return miss(name, true);
        return t->data;
    }
    // a tensor the checkpoint may leave out (nullptr, no error); if present its size must match
    const float* get_optional(const std::string& name, size_t numel) {
        const BlobTensor* t = blob.find(name);
        if (t && t->numel != numel) return miss(name, false);
        return t ? t->data : nullptr;
    }

    size_t room(size_t n) { const size_t o = host.size(); host.resize(o + al(n), 0.f); return o; }      // zeroed
    size_t push(const float* p, size_t n, size_t npad = 0) {
        const size_t o = room(std::max(n, npad));
        if (p) memcpy(host.data() + o, p, n * sizeof(float));
        return o;
    }
    // depthwise conv weight [C][k] -> tap-major [k][C]
    size_t push_tapmajor(const float* w, int C, int k) {
        const size_t o = room((size_t)C * k);
        if (w) for (int c = 0; c < C; ++c) for (int t = 0; t < k; ++t) host[o + (size_t)t * C + c] = w[(size_t)c * k + t];
        return o;
    }
    // [N][K] -> [N][Kp], columns K..Kp-1 zero
    size_t push_rows_padded(const float* w, int N, int K, int Kp) {
        const size_t o = room((size_t)N * Kp);
        if (w) for (int n = 0; n < N; ++n) memcpy(host.data() + o + (size_t)n * Kp, w + (size_t)n * K, K * sizeof(float));
        return o;
    }

    // A handle that keeps pointers binds each `const float*` field to its image offset: the field is null until finish() has
    // uploaded the image and then points at device base + offset.  The one rule: A BOUND FIELD MUST ALREADY SIT AT ITS FINAL
    // ADDRESS — a member of the heap-allocated handle, or an element of a vector that already has its final size (resize the
    // layer vectors before staging).  Never bind into a local that is copied or push_back'd afterwards.  The overloads below
    // stage like their namesakes and bind what they return.
    size_t bind(const float*& dst, size_t off) { dst = nullptr; bound_.emplace_back(&dst, off); return off; }
    size_t room(const float*& dst, size_t n) { return bind(dst, room(n)); }
    size_t push(const float*& dst, const float* p, size_t n, size_t npad = 0) { return bind(dst, push(p, n, npad)); }
    size_t push_tapmajor(const float*& dst, const float* w, int C, int k) { return bind(dst, push_tapmajor(w, C, k)); }
    size_t push_rows_padded(const float*& dst, const float* w, int N, int K, int Kp) { return bind(dst, push_rows_padded(w, N, K, Kp)); }

    // the checks (a tensor missing; with `strict`, one nobody asked for — load_state_dict(strict=True))
    int check(const char* fn, bool strict) const {
        if (!ok()) return fail(2, std::string(fn) + ": tensor missing or wrong " + (by_shape_ ? "shape: " : "size: ") + missing_);
        if (strict) {
            const std::string extra = blob.first_unused();
            if (!extra.empty()) return fail(2, std::string(fn) + ": unexpected tensor: " + extra);
        }
        return 0;
    }
    // points every bound field at `base` + its offset (host work only: `base` is wherever the image lies)
    void resolve(const float* base) const { for (const auto& b : bound_) *b.first = base + b.second; }
    // check(), then `device` is made current for the copy and the image goes to `dev`, then resolve().  Returns a TDX status;
    // nothing touches the device before the blob is accepted, and on any failure the bound fields stay null.
    int finish(const char* fn, bool strict, int device, DevBuf& dev) {
        TRY(check(fn, strict));
        DeviceGuard guard(device);
        if (guard.err != hipSuccess) return fail_hip(guard.err, __FILE__, __LINE__);
        const hipError_t e = dev.upload(host.data(), host.size() * sizeof(float));
        if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
        resolve(dev);
        return 0;
    }

private:
    std::string missing_;
    bool by_shape_ = false;
    std::vector<std::pair<const float**, size_t>> bound_;
    const float* miss(const std::string& name, bool by_shape) {
        if (missing_.empty()) { missing_ = name; by_shape_ = by_shape; }
        return nullptr;
    }
};

}  // namespace tdx
