/*
 * report.hip — the report program of a block-mode corpus scan on the device:
 * the passes of hs_report_passes.h over the scan's sorted records, with
 * hipcub's exclusive sum and stable radix sort between them, on the scan
 * context's stream.  The matches stay in HBM.
 *
 * The host side only sizes buffers, launches and reads back 8-byte totals:
 * it never reads a device array.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "vectorscan_amd.h"
#include "vsa_internal.h"
#include "hs_report_device.h"

namespace vsa_report {

namespace {

/* one thread per index, 256-thread workgroups, the index in 64 bits */
template <class F>
__global__ void __launch_bounds__(WG) report_each(uint64_t n, F f) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i < n) f(i);
}

#define REPORT_HIP(x)                   \
    do {                                \
        if ((x) != hipSuccess) {        \
            (void)hipGetLastError();    \
            return VSA_E_DEVICE;        \
        }                               \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    uint64_t bytes = 0;
};

int upload(hipStream_t s, void **d, const void *h, uint64_t bytes) {
    REPORT_HIP(hipMalloc(d, bytes ? bytes : 16));
    if (bytes) {
        REPORT_HIP(hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, s));
        REPORT_HIP(hipStreamSynchronize(s));
    }
    return VSA_OK;
}

} // namespace

struct DeviceTables {
    int device = 0;
    Tables t{};
    void *frag_off = nullptr, *pats = nullptr, *pool = nullptr;
};

int device_tables_create(vsa_ctx *ctx, const Tables &t, uint64_t pool_bytes, DeviceTables **out) {
    if (!ctx || !out) return VSA_E_INVALID;
    DeviceTables *d = new (std::nothrow) DeviceTables;
    if (!d) return VSA_E_NOMEM;
    d->device = vsa::ctxDevice(ctx);
    hipStream_t s = (hipStream_t)vsa_ctx_stream(ctx);
    int rc = hipSetDevice(d->device) == hipSuccess ? VSA_OK : VSA_E_DEVICE;
    if (!rc) rc = upload(s, &d->frag_off, t.frag_off, ((uint64_t)t.n_frags + 1) * sizeof(uint32_t));
    if (!rc) rc = upload(s, &d->pats, t.pats, (uint64_t)t.n_pats * sizeof(Pat));
    if (!rc) rc = upload(s, &d->pool, t.pool, pool_bytes);
    if (rc) {
        device_tables_free(d);
        return rc;
    }
    d->t = t;
    d->t.frag_off = (const uint32_t *)d->frag_off;
    d->t.pats = (const Pat *)d->pats;
    d->t.pool = (const uint8_t *)d->pool;
    *out = d;
    return VSA_OK;
}

void device_tables_free(DeviceTables *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipFree(d->frag_off);
    (void)hipFree(d->pats);
    (void)hipFree(d->pool);
    delete d;
}

struct DeviceReport {
    vsa_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
    Pass base{}; /* t, b, data */
    void *so = nullptr, *se = nullptr, *order = nullptr, *offsets = nullptr, *lens = nullptr;
    DevBuf slot[S_COUNT], temp;
    uint64_t *h_word = nullptr; /* pinned: the 8-byte read-backs */
    uint64_t total = 0;
    const vsa_hs_match_t *d_out = nullptr;
    const uint64_t *d_bcnt = nullptr;
    bool valid = false; /* a run's results are there */
    bool timing = false;
    int cur = ST_N;
    std::chrono::steady_clock::time_point t_cur;
    double ms[ST_N] = {0, 0, 0, 0};

    /* the backend of run_passes */
    int grow(DevBuf &b, uint64_t bytes) {
        if (b.p && bytes <= b.bytes) return VSA_OK;
        if (b.p) REPORT_HIP(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
        const uint64_t want = bytes + bytes / 4 + 256;
        REPORT_HIP(hipMalloc(&b.p, want));
        b.bytes = want;
        return VSA_OK;
    }
    template <class T>
    int buf(Slot s, uint64_t count, T **out) {
        if (count > (1ULL << 60) / sizeof(T)) return VSA_E_NOMEM;
        if (int rc = grow(slot[s], count * sizeof(T))) return rc;
        *out = (T *)slot[s].p;
        return VSA_OK;
    }
    template <class F>
    int each(uint64_t n, const F &f) {
        if (!n) return VSA_OK;
        const uint64_t g = grid_for(n);
        if (!g) return VSA_E_INVALID;
        hipLaunchKernelGGL(report_each<F>, dim3((uint32_t)g), dim3(WG), 0, stream, n, f);
        REPORT_HIP(hipGetLastError());
        return VSA_OK;
    }
    int exclusive_sum(const uint64_t *in, uint64_t *out, uint64_t n) {
        size_t bytes = 0;
        REPORT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, stream));
        if (int rc = grow(temp, bytes)) return rc;
        bytes = temp.bytes;
        REPORT_HIP(hipcub::DeviceScan::ExclusiveSum(temp.p, bytes, in, out, n, stream));
        return VSA_OK;
    }
    int sort_pairs(const uint64_t *kin, uint64_t *kout, const uint64_t *vin, uint64_t *vout,
                   uint64_t n, int end_bit) {
        size_t bytes = 0;
        REPORT_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout, n, 0,
                                                      end_bit, stream));
        if (int rc = grow(temp, bytes)) return rc;
        bytes = temp.bytes;
        REPORT_HIP(hipcub::DeviceRadixSort::SortPairs(temp.p, bytes, kin, kout, vin, vout, n, 0,
                                                      end_bit, stream));
        return VSA_OK;
    }
    int read_u64(const uint64_t *src, uint64_t *dst) {
        REPORT_HIP(hipMemcpyAsync(h_word, src, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        REPORT_HIP(hipStreamSynchronize(stream));
        *dst = *h_word;
        return VSA_OK;
    }
    void stage(Stage s) {
        if (!timing) return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        if (cur != ST_N) ms[cur] += std::chrono::duration<double, std::milli>(now - t_cur).count();
        cur = s;
        t_cur = now;
    }
};

int device_report_create(vsa_ctx *ctx, const DeviceTables *tabs, const BlockTable &bt,
                         const uint64_t *offsets, const uint64_t *lens, uint32_t nblocks,
                         const uint8_t *d_data, DeviceReport **out) {
    if (!ctx || !tabs || !out) return VSA_E_INVALID;
    DeviceReport *r = new (std::nothrow) DeviceReport;
    if (!r) return VSA_E_NOMEM;
    r->ctx = ctx;
    r->stream = (hipStream_t)vsa_ctx_stream(ctx);
    r->device = vsa::ctxDevice(ctx);
    r->timing = getenv("VSA_HOST_TIMING") != nullptr;
    const uint64_t npos = bt.so.size();
    int rc = hipSetDevice(r->device) == hipSuccess ? VSA_OK : VSA_E_DEVICE;
    if (!rc) rc = upload(r->stream, &r->so, bt.so.data(), npos * sizeof(uint64_t));
    if (!rc) rc = upload(r->stream, &r->se, bt.se.data(), npos * sizeof(uint64_t));
    if (!rc) rc = upload(r->stream, &r->order, bt.order.data(), npos * sizeof(uint32_t));
    if (!rc) rc = upload(r->stream, &r->offsets, offsets, (uint64_t)nblocks * sizeof(uint64_t));
    if (!rc) rc = upload(r->stream, &r->lens, lens, (uint64_t)nblocks * sizeof(uint64_t));
    if (!rc && hipHostMalloc((void **)&r->h_word, sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        r->h_word = nullptr;
        rc = VSA_E_NOMEM;
    }
    if (rc) {
        device_report_free(r);
        return rc;
    }
    r->base.t = tabs->t;
    r->base.b.so = (const uint64_t *)r->so;
    r->base.b.se = (const uint64_t *)r->se;
    r->base.b.order = (const uint32_t *)r->order;
    r->base.b.offsets = (const uint64_t *)r->offsets;
    r->base.b.lens = (const uint64_t *)r->lens;
    r->base.b.npos = (uint32_t)npos;
    r->base.b.nblocks = nblocks;
    r->base.b.uniform = bt.uniform;
    r->base.b.off0 = bt.off0;
    r->base.b.ulen = bt.ulen;
    r->base.data = d_data;
    *out = r;
    return VSA_OK;
}

void device_report_free(DeviceReport *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    for (void *p : {r->so, r->se, r->order, r->offsets, r->lens, r->temp.p}) (void)hipFree(p);
    for (DevBuf &b : r->slot) (void)hipFree(b.p);
    if (r->h_word) (void)hipHostFree(r->h_word);
    delete r;
}

int device_report_run(DeviceReport *r, const uint64_t *d_keys, const uint32_t *d_ids, uint64_t n,
                      uint64_t *counts, uint64_t *total) {
    if (!r || !total || (n && (!d_keys || !d_ids))) return VSA_E_INVALID;
    REPORT_HIP(hipSetDevice(r->device));
    r->valid = false;
    r->total = 0;
    Pass p = r->base;
    p.keys = d_keys;
    p.ids = d_ids;
    p.n = n;
    for (double &m : r->ms) m = 0;
    r->cur = ST_N;
    if (int rc = run_passes(*r, p, total)) return rc;
    REPORT_HIP(hipStreamSynchronize(r->stream));
    if (counts && p.b.nblocks) {
        REPORT_HIP(hipMemcpyAsync(counts, p.bcnt, (uint64_t)p.b.nblocks * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, r->stream));
        REPORT_HIP(hipStreamSynchronize(r->stream));
    }
    r->total = *total;
    r->d_out = p.out;
    r->d_bcnt = p.bcnt;
    r->valid = true;
    if (r->timing)
        fprintf(stderr, "device_report: %llu records, %llu candidates, %llu matches: lead %.3f ms, "
                "exhaustion %.3f ms, count %.3f ms, emit %.3f ms\n", (unsigned long long)n,
                (unsigned long long)p.ncand, (unsigned long long)*total, r->ms[ST_LEAD],
                r->ms[ST_EXHAUST], r->ms[ST_COUNT], r->ms[ST_EMIT]);
    return VSA_OK;
}

int device_report_matches(DeviceReport *r, const vsa_hs_match_t **d_matches, uint64_t *n) {
    if (!r || !r->valid) return VSA_E_INVALID;
    if (d_matches) *d_matches = r->d_out;
    if (n) *n = r->total;
    return VSA_OK;
}

int device_report_copy(DeviceReport *r, vsa_hs_match_t *out, uint64_t n) {
    if (!r || !r->valid || n > r->total || (n && !out)) return VSA_E_INVALID;
    if (!n) return VSA_OK;
    REPORT_HIP(hipSetDevice(r->device));
    REPORT_HIP(hipMemcpyAsync(out, r->d_out, n * sizeof(vsa_hs_match_t), hipMemcpyDeviceToHost,
                              r->stream));
    REPORT_HIP(hipStreamSynchronize(r->stream));
    return VSA_OK;
}

} // namespace vsa_report
