// C ABI entry points (include/bzh2.h): context, base tables, host<->device
// staging around the MSM / NTT drivers, and the host-side helpers.
#include <cstring>
#include <algorithm>
#include <thread>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "curve.cuh"
#include "host_field.hpp"
#include "vm2_isa.hpp"

using namespace bzh;

static bool valid_curve(int c) { return c >= 0 && c <= 2; }
static bool valid_field(int f) { return f >= 0 && f <= 3; }
static bool valid_form(int f) { return f == BZH_FORM_CANONICAL || f == BZH_FORM_MONTGOMERY; }
static bool valid_mem(int m) { return m == BZH_MEM_HOST || m == BZH_MEM_DEVICE; }
static unsigned field_two_adicity(int f) {
    unsigned s = 0;
    with_field(f, [&](auto p) {
        s = FieldInfo<decltype(p)>::S;
        return BZH_OK;
    });
    return s;
}

// ---- host helpers (CPU build of the same field templates) ------------------
namespace {
// Staging for BZH_MEM_HOST calls: carve device buffers out of WS_STAGE, copy in, and (canonical form) convert to Montgomery on
// the device.  The buffers live until the call returns; what runs on them (msm_run*, ntt_run*, poly_*, lookup_permute, ipa_open)
// takes other slots only.
struct Stager {
    bzh_ctx* ctx;
    int field, form;
    char* cur = nullptr;
    int begin(size_t total_bytes) {
        void* p = nullptr;
        int rc = ws_ensure(ctx, WS_STAGE, total_bytes + 256, &p);
        cur = (char*)p;
        return rc;
    }
    uint32_t* carve(size_t bytes) {
        uint32_t* p = (uint32_t*)cur;
        cur += (bytes + 63) & ~(size_t)63;
        return p;
    }
    int in(const void* host, size_t elems, uint32_t** dev) {
        *dev = carve(elems * 32);
        if (!elems) return BZH_OK;
        int rc = h2d_small(ctx, *dev, host, elems * 32);
        if (rc) return rc;
        if (form == BZH_FORM_CANONICAL) return field_convert(ctx, field, *dev, elems, 1);
        return BZH_OK;
    }
    int out(void* host, uint32_t* dev, size_t elems) {
        if (!elems) return BZH_OK;
        if (form == BZH_FORM_CANONICAL) {
            int rc = field_convert(ctx, field, dev, elems, 0);
            if (rc) return rc;
        }
        int rc = d2h_async(ctx, host, dev, elems * 32);
        if (rc) return rc;
        return d2h_finish(ctx);
    }
};

// sum of n Jacobian points on the host: the combine step of an MSM whose points are split over several GPUs
// (each rank's partial result is one 96-byte point; SURVEY.md section 8e "8-GPU single MSM")
template <class P>
static void jac_sum_host(const uint64_t* xyz, size_t n, int form, uint64_t* out) {
    std::vector<uint64_t> aff(8 * (n ? n : 1));
    h_jac_to_affine<P>(xyz, n, form, form, aff.data());
    Xyzz<P> acc = xyzz_identity<P>();
    for (size_t i = 0; i < n; i++) {
        Affine<P> a;
        a.x = fe_from_u64<P>(aff.data() + 8 * i, form);
        a.y = fe_from_u64<P>(aff.data() + 8 * i + 4, form);
        if (aff_is_id(a)) continue;
        xyzz_madd(acc, a);
    }
    Fe<P> X, Y, Z;
    xyzz_to_jacobian(acc, X, Y, Z);
    fe_to_u64<P>(out, X, form);
    fe_to_u64<P>(out + 4, Y, form);
    fe_to_u64<P>(out + 8, Z, form);
}

template <class PP>
static int permute_pair_host(const uint64_t* input, const uint64_t* table, size_t usable, int form, uint64_t* out_input,
                             uint64_t* out_table) {
    // canonical values as sortable keys (pasta_curves orders field elements by canonical value)
    struct Key {
        uint64_t l[4];
        bool operator<(const Key& o) const {
            for (int i = 3; i >= 0; i--)
                if (l[i] != o.l[i]) return l[i] < o.l[i];
            return false;
        }
        bool operator==(const Key& o) const { return !memcmp(l, o.l, 32); }
    };
    std::vector<Key> a(usable), t(usable);
    if (form == BZH_FORM_CANONICAL) {  // canonical limbs ARE the sort keys: no field arithmetic on the host
        memcpy(a.data(), input, usable * 32);
        memcpy(t.data(), table, usable * 32);
    } else {
        for (size_t i = 0; i < usable; i++) {
            fe_to_u64<PP>(a[i].l, fe_from_u64<PP>(input + 4 * i, form), BZH_FORM_CANONICAL);
            fe_to_u64<PP>(t[i].l, fe_from_u64<PP>(table + 4 * i, form), BZH_FORM_CANONICAL);
        }
    }
    // values below 2^64 (range tables, compressed small columns -- the reference's lookups): sort the low limbs as integers
    auto is_small = [](const std::vector<Key>& v) {
        for (const Key& k : v)
            if (k.l[1] | k.l[2] | k.l[3]) return false;
        return true;
    };
    const bool small_a = is_small(a), small_t = is_small(t);
    auto sort_keys = [](std::vector<Key>& v, bool small) {
        if (!small) {
            std::sort(v.begin(), v.end());
            return;
        }
        uint64_t mx = 0;
        for (const Key& k : v) mx = std::max(mx, k.l[0]);
        if (mx < 65536 && v.size() >= 256) {   // a histogram does it (10-bit range table: 1 024 distinct values)
            std::vector<uint32_t> cnt(mx + 1, 0);
            for (const Key& k : v) cnt[k.l[0]]++;
            size_t at = 0;
            for (uint64_t val = 0; val <= mx; val++)
                for (uint32_t c = cnt[val]; c; c--) v[at++].l[0] = val;
            return;
        }
        std::vector<uint64_t> lo(v.size());
        for (size_t i = 0; i < v.size(); i++) lo[i] = v[i].l[0];
        std::sort(lo.begin(), lo.end());
        for (size_t i = 0; i < v.size(); i++) v[i].l[0] = lo[i];
    };
    if (usable >= 4096 && !(small_a && small_t)) {  // the two sorts are independent: a second thread takes the table
        std::thread other([&]() { sort_keys(t, small_t); });
        sort_keys(a, small_a);
        other.join();
    } else {   // (integer / histogram sorts take less than starting a thread does)
        sort_keys(a, small_a);
        sort_keys(t, small_t);
    }
    // leftover multiset = table minus one copy of every distinct input value
    std::vector<Key> s(usable);
    std::vector<size_t> repeated;
    std::vector<char> used(usable, 0);
    size_t tp = 0;
    for (size_t i = 0; i < usable; i++) {
        if (i == 0 || !(a[i] == a[i - 1])) {
            while (tp < usable && t[tp] < a[i]) tp++;
            if (tp >= usable || !(t[tp] == a[i])) return BZH_E_RANGE;  // input value not in the table
            used[tp++] = 1;
            s[i] = a[i];
        } else {
            repeated.push_back(i);
        }
    }
    for (size_t j = 0; j < usable; j++) {  // ascending leftovers go to the repeated rows from the last one backwards
        if (used[j]) continue;
        if (repeated.empty()) return BZH_E_RANGE;
        s[repeated.back()] = t[j];
        repeated.pop_back();
    }
    if (form == BZH_FORM_CANONICAL) {
        memcpy(out_input, a.data(), usable * 32);
        memcpy(out_table, s.data(), usable * 32);
        return BZH_OK;
    }
    for (size_t i = 0; i < usable; i++) {
        fe_to_u64<PP>(out_input + 4 * i, fe_from_u64<PP>(a[i].l, BZH_FORM_CANONICAL), form);
        fe_to_u64<PP>(out_table + 4 * i, fe_from_u64<PP>(s[i].l, BZH_FORM_CANONICAL), form);
    }
    return BZH_OK;
}

}  // namespace

extern "C" {

const char* bzh_version(void) { return "bzh2 0.1 (gfx950)"; }

const char* bzh_strerror(int status) {
    switch (status) {
        case BZH_OK: return "ok";
        case BZH_E_ARG: return "invalid argument";
        case BZH_E_OOM: return "out of memory";
        case BZH_E_HIP: return "HIP runtime error";
        case BZH_E_RANGE: return "value out of range";
        case BZH_E_NOGPU: return "no usable GPU";
        case BZH_E_VERIFY: return "proof does not verify";
    }
    return "unknown status";
}

int bzh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int ctx_create_common(int device, void* stream, bool own, bzh_ctx** out) {
    if (!out) return BZH_E_ARG;
    *out = nullptr;
    int n = bzh_device_count();
    if (n <= 0) return BZH_E_NOGPU;
    if (device < 0 || device >= n) return BZH_E_ARG;
    bzh_ctx* ctx = new (std::nothrow) bzh_ctx();
    if (!ctx) return BZH_E_OOM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) {
        delete ctx;
        return BZH_E_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cu = prop.multiProcessorCount;
    if (own) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            delete ctx;
            return BZH_E_HIP;
        }
        ctx->own_stream = true;
    } else {
        ctx->stream = (hipStream_t)stream;
    }
    *out = ctx;
    return BZH_OK;
}

int bzh_ctx_create(int device, bzh_ctx** out) { return ctx_create_common(device, nullptr, true, out); }
int bzh_ctx_create_on_stream(int device, void* hip_stream, bzh_ctx** out) {
    return ctx_create_common(device, hip_stream, false, out);
}

int bzh_ctx_destroy(bzh_ctx* ctx) {
    if (!ctx) return BZH_E_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->ntt.reset();
    for (int i = 0; i < kWsSlots; i++)
        if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
    if (ctx->d_add_counter) (void)hipFree(ctx->d_add_counter);
    if (ctx->ped_tbl) (void)hipFree(ctx->ped_tbl);
    if (ctx->syn_tbl) (void)hipFree(ctx->syn_tbl);
    for (uint32_t* t : ctx->sqrt_tbl)
        if (t) (void)hipFree(t);
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->pin_big) (void)hipHostFree(ctx->pin_big);
    for (auto& s : ctx->spans) {
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
    }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return BZH_OK;
}

int bzh_ctx_sync(bzh_ctx* ctx) {
    if (!ctx) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BZH_OK;
}

const char* bzh_last_error(const bzh_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

static int drain_spans(bzh_ctx* ctx) {
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& s : ctx->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            ctx->acc_ms[s.cls] += ms;
            ctx->acc_n[s.cls] += 1;
        }
        ctx->event_pool.push_back(s.a);
        ctx->event_pool.push_back(s.b);
    }
    ctx->spans.clear();
    return BZH_OK;
}

int bzh_ctx_profile(bzh_ctx* ctx, int enable) {
    if (!ctx) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = drain_spans(ctx);
    if (rc) return rc;
    for (int i = 0; i < BZH_T_COUNT; i++) {
        ctx->acc_ms[i] = 0;
        ctx->acc_n[i] = 0;
        ctx->alg_bytes[i] = 0;
    }
    if (enable && !ctx->d_add_counter) {
        BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
        BZH_HIP_TRY(ctx, hipMalloc((void**)&ctx->d_add_counter, 8));
    }
    if (ctx->d_add_counter) BZH_HIP_TRY(ctx, hipMemsetAsync(ctx->d_add_counter, 0, 8, ctx->stream));
    ctx->profiling = enable != 0;
    return BZH_OK;
}

int bzh_ctx_msm_additions(bzh_ctx* ctx, uint64_t* additions) {
    if (!ctx || !additions) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    *additions = 0;
    if (!ctx->d_add_counter) return BZH_OK;
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long v = 0;
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    BZH_HIP_TRY(ctx, hipMemcpy(&v, ctx->d_add_counter, 8, hipMemcpyDeviceToHost));
    *additions = v;
    return BZH_OK;
}

int bzh_ctx_work(bzh_ctx* ctx, double* algorithmic_bytes) {
    if (!ctx || !algorithmic_bytes) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int i = 0; i < BZH_T_COUNT; i++) algorithmic_bytes[i] = ctx->alg_bytes[i];
    return BZH_OK;
}

int bzh_ctx_timings(bzh_ctx* ctx, double* ms, uint64_t* launches) {
    if (!ctx || !ms || !launches) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = drain_spans(ctx);
    if (rc) return rc;
    for (int i = 0; i < BZH_T_COUNT; i++) {
        ms[i] = ctx->acc_ms[i];
        launches[i] = ctx->acc_n[i];
    }
    return BZH_OK;
}

int bzh_bases_upload(bzh_ctx* ctx, int curve, const uint64_t* xy, size_t n, int form, int mem, bzh_bases** out) {
    if (!ctx || !out || (!xy && n) || !valid_curve(curve) || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    bzh_bases* b = new (std::nothrow) bzh_bases();
    if (!b) return BZH_E_OOM;
    b->curve = curve;
    b->n = n;
    b->device = ctx->device;
    hipError_t e = hipMalloc((void**)&b->d_xy, (n ? n : 1) * 64);
    if (e != hipSuccess) {
        delete b;
        ctx->last_error = std::string("hipMalloc(bases): ") + hipGetErrorString(e);
        return BZH_E_OOM;
    }
    e = hipMemcpyAsync(b->d_xy, xy, n * 64, mem == BZH_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                       ctx->stream);
    int rc = BZH_OK;
    if (e != hipSuccess) {
        ctx->last_error = std::string("hipMemcpyAsync(bases): ") + hipGetErrorString(e);
        rc = BZH_E_HIP;
    }
    if (!rc && form == BZH_FORM_CANONICAL) rc = bases_to_montgomery(ctx, curve, b->d_xy, n);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = BZH_E_HIP;
    if (rc) {
        (void)hipFree(b->d_xy);
        delete b;
        return rc;
    }
    *out = b;
    return BZH_OK;
}

int bzh_bases_free(bzh_ctx* ctx, bzh_bases* bases) {
    if (!ctx || !bases) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(bases->d_xy);
    if (bases->d_xy29) (void)hipFree(bases->d_xy29);
    delete bases;
    return BZH_OK;
}

size_t bzh_bases_len(const bzh_bases* bases) { return bases ? bases->n : 0; }

int bzh_bases_precompute(bzh_ctx* ctx, bzh_bases* bases, int window_bits) {
    if (!ctx || !bases || window_bits < 0) return BZH_E_ARG;
    if (bases->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bases_precompute(ctx, bases, window_bits);
}

int bzh_msm(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* scalars, size_t n, size_t batch, int form, int mem,
            uint64_t* out_xyz) {
    if (!ctx || !bases || !out_xyz || (!scalars && n && batch) || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    if (n > bases->n) return BZH_E_ARG;  // halo2: assert_eq!(coeffs.len(), bases.len())
    if (bases->device != ctx->device) return BZH_E_ARG;
    if (batch == 0) return BZH_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE) return msm_run(ctx, bases, (const uint32_t*)scalars, n, batch, form, (uint32_t*)out_xyz);
    void* stage = nullptr;
    const size_t sbytes = batch * n * 32, obytes = batch * 96;
    int rc = ws_ensure(ctx, WS_STAGE, sbytes + obytes + 64, &stage);   // held across msm_run, which takes WS_SCRATCH_* only
    if (rc) return rc;
    uint32_t* d_s = (uint32_t*)stage;
    uint32_t* d_o = (uint32_t*)((char*)stage + ((sbytes + 63) & ~(size_t)63));
    if (sbytes) BZH_HIP_TRY(ctx, hipMemcpyAsync(d_s, scalars, sbytes, hipMemcpyHostToDevice, ctx->stream));
    rc = msm_run(ctx, bases, d_s, n, batch, form, d_o);
    if (rc) return rc;
    BZH_HIP_TRY(ctx, hipMemcpyAsync(out_xyz, d_o, obytes, hipMemcpyDeviceToHost, ctx->stream));
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BZH_OK;
}

int bzh_ntt(bzh_ctx* ctx, int field, uint64_t* data, unsigned log_n, size_t batch, const uint64_t* omega,
            const uint64_t* coset_shift, int inverse, int form, int mem) {
    if (!ctx || !data || !omega || !valid_field(field) || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    if (log_n > field_two_adicity(field) || log_n > 30) return BZH_E_RANGE;
    if (batch == 0) return BZH_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mem == BZH_MEM_DEVICE) return ntt_run(ctx, field, (uint32_t*)data, log_n, batch, omega, coset_shift, inverse, form);
    void* stage = nullptr;
    const size_t bytes = (batch << log_n) * 32;
    int rc = ws_ensure(ctx, WS_STAGE, bytes, &stage);   // held across ntt_run, which takes WS_SCRATCH_A only
    if (rc) return rc;
    BZH_HIP_TRY(ctx, hipMemcpyAsync(stage, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = ntt_run(ctx, field, (uint32_t*)stage, log_n, batch, omega, coset_shift, inverse, form);
    if (rc) return rc;
    BZH_HIP_TRY(ctx, hipMemcpyAsync(data, stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BZH_OK;
}

int bzh_coeff_to_extended(bzh_ctx* ctx, int field, const uint64_t* coeffs, unsigned log_n, uint64_t* out, unsigned log_ext,
                          size_t batch, const uint64_t* omega_ext, const uint64_t* coset_shift, int form, int mem) {
    if (!ctx || !coeffs || !out || !omega_ext || !valid_field(field) || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    if (log_ext > field_two_adicity(field) || log_ext > 30 || log_n > log_ext) return BZH_E_RANGE;
    if (batch == 0) return BZH_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t in_elems = batch << log_n, out_elems = batch << log_ext;
    const uint32_t* d_in = (const uint32_t*)coeffs;
    uint32_t* d_out = (uint32_t*)out;
    void* stage = nullptr;
    if (mem == BZH_MEM_HOST || form == BZH_FORM_CANONICAL) {
        // staged copy of the coefficients (host memory, or canonical device input that may not be written to); held across
        // ntt_run_padded, which takes WS_SCRATCH_A only
        int rc = ws_ensure(ctx, WS_STAGE, (in_elems + (mem == BZH_MEM_HOST ? out_elems : 0)) * 32, &stage);
        if (rc) return rc;
        BZH_HIP_TRY(ctx, hipMemcpyAsync(stage, coeffs, in_elems * 32, mem == BZH_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                        ctx->stream));
        d_in = (const uint32_t*)stage;
        if (mem == BZH_MEM_HOST) d_out = (uint32_t*)stage + in_elems * 8;
        if (form == BZH_FORM_CANONICAL) {
            rc = field_convert(ctx, field, (uint32_t*)stage, in_elems, 1);
            if (rc) return rc;
        }
    }
    uint64_t w[4], sh[4];
    memcpy(w, omega_ext, 32);
    if (coset_shift) memcpy(sh, coset_shift, 32);
    if (form == BZH_FORM_CANONICAL) {
        BZH_TRY(with_field(field, [&](auto p) {   // 4 host limbs, canonical -> Montgomery in place
            using P = decltype(p);
            fe_to_u64<P>(w, fe_from_u64<P>(w, BZH_FORM_CANONICAL));
            if (coset_shift) fe_to_u64<P>(sh, fe_from_u64<P>(sh, BZH_FORM_CANONICAL));
            return BZH_OK;
        }));
    }
    int rc = ntt_run_padded(ctx, field, d_out, d_in, log_n, log_ext, batch, w, coset_shift ? sh : nullptr);
    if (rc) return rc;
    if (form == BZH_FORM_CANONICAL) {
        rc = field_convert(ctx, field, d_out, out_elems, 0);
        if (rc) return rc;
    }
    if (mem == BZH_MEM_HOST) {
        BZH_HIP_TRY(ctx, hipMemcpyAsync(out, d_out, out_elems * 32, hipMemcpyDeviceToHost, ctx->stream));
        BZH_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return BZH_OK;
}

#define BZH_POLY_PROLOGUE(cond_args)                                                            \
    if (!ctx || !valid_field(field) || !valid_form(form) || !valid_mem(mem) || (cond_args)) return BZH_E_ARG; \
    std::lock_guard<std::mutex> lk(ctx->mu);                                                    \
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));                                                \
    int rc = BZH_OK;                                                                            \
    (void)rc

int bzh_field_convert(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int to_montgomery, int mem) {
    const int form = BZH_FORM_MONTGOMERY;
    BZH_POLY_PROLOGUE(!data && count);
    if (!count) return BZH_OK;
    if (mem == BZH_MEM_DEVICE) return field_convert(ctx, field, (uint32_t*)data, count, to_montgomery ? 1 : 0);
    Stager s{ctx, field, BZH_FORM_MONTGOMERY};
    uint32_t* d;
    if ((rc = s.begin(count * 32))) return rc;
    if ((rc = s.in(data, count, &d))) return rc;
    if ((rc = field_convert(ctx, field, d, count, to_montgomery ? 1 : 0))) return rc;
    return s.out(data, d, count);
}

int bzh_random_field(bzh_ctx* ctx, int field, const uint8_t* rng_bytes, size_t count, int form, int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE((!rng_bytes || !out) && count);
    if (!count) return BZH_OK;
    Stager s{ctx, field, BZH_FORM_MONTGOMERY};
    if ((rc = s.begin(count * 64 + (mem == BZH_MEM_HOST ? count * 32 : 0) + 256))) return rc;
    uint32_t* d_raw = s.carve(count * 64);
    BZH_HIP_TRY(ctx, hipMemcpyAsync(d_raw, rng_bytes, count * 64, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* d_out = mem == BZH_MEM_HOST ? s.carve(count * 32) : (uint32_t*)out;
    if ((rc = random_field(ctx, field, d_raw, count, d_out))) return rc;
    if (form == BZH_FORM_CANONICAL && (rc = field_convert(ctx, field, d_out, count, 0))) return rc;
    if (mem == BZH_MEM_HOST) {
        Stager so{ctx, field, BZH_FORM_MONTGOMERY};  // already in the requested form: plain copy out
        return so.out(out, d_out, count);
    }
    return BZH_OK;  // staging reuse by the next call is stream-ordered
}

int bzh_batch_invert(bzh_ctx* ctx, int field, uint64_t* data, size_t count, int form, int mem) {
    BZH_POLY_PROLOGUE(!data && count);
    if (!count) return BZH_OK;
    if (mem == BZH_MEM_DEVICE) {
        uint32_t* d = (uint32_t*)data;
        if (form == BZH_FORM_CANONICAL && (rc = field_convert(ctx, field, d, count, 1))) return rc;
        if ((rc = poly_batch_invert(ctx, field, d, count))) return rc;
        if (form == BZH_FORM_CANONICAL) rc = field_convert(ctx, field, d, count, 0);
        return rc;
    }
    Stager s{ctx, field, form};
    uint32_t* d;
    if ((rc = s.begin(count * 32))) return rc;
    if ((rc = s.in(data, count, &d))) return rc;
    if ((rc = poly_batch_invert(ctx, field, d, count))) return rc;
    return s.out(data, d, count);
}

int bzh_prefix_product(bzh_ctx* ctx, int field, uint64_t* data, size_t n, size_t batch, int form, int mem) {
    BZH_POLY_PROLOGUE(!data && n && batch);
    const size_t count = n * batch;
    if (!count) return BZH_OK;
    if (mem == BZH_MEM_DEVICE) {
        uint32_t* d = (uint32_t*)data;
        if (form == BZH_FORM_CANONICAL && (rc = field_convert(ctx, field, d, count, 1))) return rc;
        if ((rc = poly_prefix_product(ctx, field, d, n, batch))) return rc;
        if (form == BZH_FORM_CANONICAL) rc = field_convert(ctx, field, d, count, 0);
        return rc;
    }
    Stager s{ctx, field, form};
    uint32_t* d;
    if ((rc = s.begin(count * 32))) return rc;
    if ((rc = s.in(data, count, &d))) return rc;
    if ((rc = poly_prefix_product(ctx, field, d, n, batch))) return rc;
    return s.out(data, d, count);
}

int bzh_eval_polynomial(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, size_t batch, const uint64_t* xs, size_t nx,
                        int form, int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE(!coeffs || !xs || !out || !n || (nx != 1 && nx != batch));
    if (!batch) return BZH_OK;
    const size_t stride = nx == 1 ? 0 : 1;
    if (mem == BZH_MEM_DEVICE) {
        if (form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return poly_eval(ctx, field, (const uint32_t*)coeffs, n, batch, (const uint32_t*)xs, stride, (uint32_t*)out);
    }
    Stager s{ctx, field, form};
    uint32_t *dc, *dx;
    if ((rc = s.begin((n * batch + nx + batch) * 32 + 256))) return rc;
    if ((rc = s.in(coeffs, n * batch, &dc))) return rc;
    if ((rc = s.in(xs, nx, &dx))) return rc;
    uint32_t* dout = s.carve(batch * 32);
    if ((rc = poly_eval(ctx, field, dc, n, batch, dx, stride, dout))) return rc;
    return s.out(out, dout, batch);
}

int bzh_inner_product(bzh_ctx* ctx, int field, const uint64_t* a, const uint64_t* b, size_t n, size_t batch, int form, int mem,
                      uint64_t* out) {
    BZH_POLY_PROLOGUE(!a || !b || !out || !n);
    if (!batch) return BZH_OK;
    if (mem == BZH_MEM_DEVICE) {
        if (form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return poly_inner_product(ctx, field, (const uint32_t*)a, (const uint32_t*)b, n, batch, (uint32_t*)out);
    }
    Stager s{ctx, field, form};
    uint32_t *da, *db;
    if ((rc = s.begin((2 * n * batch + batch) * 32 + 256))) return rc;
    if ((rc = s.in(a, n * batch, &da))) return rc;
    if ((rc = s.in(b, n * batch, &db))) return rc;
    uint32_t* dout = s.carve(batch * 32);
    if ((rc = poly_inner_product(ctx, field, da, db, n, batch, dout))) return rc;
    return s.out(out, dout, batch);
}

int bzh_fold(bzh_ctx* ctx, int field, const uint64_t* in, size_t half, size_t batch, const uint64_t* u, size_t nu, int form,
             int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE(!in || !u || !out || (nu != 1 && nu != batch));
    if (!batch || !half) return BZH_OK;
    const size_t stride = nu == 1 ? 0 : 1;
    if (mem == BZH_MEM_DEVICE) {
        if (form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return poly_fold(ctx, field, (const uint32_t*)in, half, batch, (const uint32_t*)u, stride, (uint32_t*)out);
    }
    Stager s{ctx, field, form};
    uint32_t *din, *du;
    if ((rc = s.begin((3 * half * batch + nu) * 32 + 256))) return rc;
    if ((rc = s.in(in, 2 * half * batch, &din))) return rc;
    if ((rc = s.in(u, nu, &du))) return rc;
    uint32_t* dout = s.carve(half * batch * 32);
    if ((rc = poly_fold(ctx, field, din, half, batch, du, stride, dout))) return rc;
    return s.out(out, dout, half * batch);
}

int bzh_vec_mul(bzh_ctx* ctx, int field, uint64_t* a, const uint64_t* b, size_t count, int form, int mem) {
    BZH_POLY_PROLOGUE((!a || !b) && count);
    if (!count) return BZH_OK;
    if (mem == BZH_MEM_DEVICE) {
        if (form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return poly_vec_mul(ctx, field, (uint32_t*)a, (const uint32_t*)b, count);
    }
    Stager s{ctx, field, form};
    uint32_t *da, *db;
    if ((rc = s.begin(2 * count * 32 + 256))) return rc;
    if ((rc = s.in(a, count, &da))) return rc;
    if ((rc = s.in(b, count, &db))) return rc;
    if ((rc = poly_vec_mul(ctx, field, da, db, count))) return rc;
    return s.out(a, da, count);
}

int bzh_kate_division_batch(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, size_t batch, const uint64_t* xs, int form,
                            int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE(!coeffs || !xs || !out || n < 1 || !batch || batch > 65535);
    if (n == 1) return BZH_OK;
    if (mem == BZH_MEM_DEVICE && form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
    // x_v per vector, uploaded in Montgomery form
    std::vector<uint64_t> xh(batch * 4);
    with_field(field, [&](auto p) {
        using PP = decltype(p);
        for (size_t v = 0; v < batch; v++) fe_to_u64<PP>(xh.data() + v * 4, fe_from_u64<PP>(xs + 4 * v, form));
        return BZH_OK;
    });
    Stager s{ctx, field, BZH_FORM_MONTGOMERY};
    if ((rc = s.begin(((mem == BZH_MEM_HOST ? 2 * n : 0) + 1) * batch * 32 + 512))) return rc;
    uint32_t* d_x;
    if ((rc = s.in(xh.data(), batch, &d_x))) return rc;
    if (mem == BZH_MEM_HOST) {
        Stager sc{ctx, field, form};
        sc.cur = s.cur;
        uint32_t* d_c;
        if ((rc = sc.in(coeffs, n * batch, &d_c))) return rc;
        uint32_t* d_q = sc.carve((n - 1) * batch * 32);
        if ((rc = poly_kate_division(ctx, field, d_c, n, batch, d_x, d_q))) return rc;
        return sc.out(out, d_q, (n - 1) * batch);
    }
    rc = poly_kate_division(ctx, field, (const uint32_t*)coeffs, n, batch, d_x, (uint32_t*)out);
    return rc;  // staging reuse by the next call is stream-ordered
}

int bzh_kate_division(bzh_ctx* ctx, int field, const uint64_t* coeffs, size_t n, const uint64_t* x, int form, int mem,
                      uint64_t* out) {
    return bzh_kate_division_batch(ctx, field, coeffs, n, 1, x, form, mem, out);
}

int bzh_permute_expression_pair(int field, const uint64_t* input, const uint64_t* table, size_t usable_rows, int form,
                                uint64_t* out_input, uint64_t* out_table) {
    if (!valid_field(field) || !valid_form(form) || ((!input || !table || !out_input || !out_table) && usable_rows)) return BZH_E_ARG;
    return with_field(field, [&](auto p) { return permute_pair_host<decltype(p)>(input, table, usable_rows, form, out_input, out_table); });
}

int bzh_permute_expression_pair_batch(bzh_ctx* ctx, int field, const uint64_t* input, const uint64_t* table, size_t stride, size_t usable_rows,
                                      size_t batch, int form, int mem, uint64_t* out_input, uint64_t* out_table, int32_t* status) {
    BZH_POLY_PROLOGUE(!input || !table || !out_input || !out_table || !usable_rows || usable_rows > stride || !batch || batch > 32767 ||
                      stride >> 31);
    void* ws = nullptr;
    // leaf scratch: lookup_permute's kernels work in it and call no MSM; the staging below is WS_STAGE
    if ((rc = ws_ensure(ctx, WS_SCRATCH_B, lookup_permute_ws_bytes(usable_rows, batch), &ws))) return rc;
    const size_t total = batch * stride;
    const uint32_t *d_in = (const uint32_t*)input, *d_tab = (const uint32_t*)table;
    uint32_t *d_oa = (uint32_t*)out_input, *d_os = (uint32_t*)out_table;
    Stager s{ctx, field, BZH_FORM_MONTGOMERY};  // (raw copies: the kernels read and write either form)
    if (mem == BZH_MEM_HOST) {
        uint32_t *di, *dt;
        if ((rc = s.begin(4 * total * 32 + 1024))) return rc;
        if ((rc = s.in(input, total, &di))) return rc;
        if ((rc = s.in(table, total, &dt))) return rc;
        d_in = di;
        d_tab = dt;
        d_oa = s.carve(total * 32);
        d_os = s.carve(total * 32);
    }
    int32_t* d_status = nullptr;
    if ((rc = lookup_permute(ctx, field, d_in, d_tab, stride, usable_rows, batch, form, d_oa, d_os, stride, stride, ws, &d_status))) return rc;
    std::vector<int32_t> st(batch, 0);
    if ((rc = d2h_async(ctx, st.data(), d_status, batch * sizeof(int32_t)))) return rc;
    if (mem == BZH_MEM_HOST) {
        if ((rc = d2h_async(ctx, out_input, d_oa, total * 32))) return rc;
        if ((rc = d2h_async(ctx, out_table, d_os, total * 32))) return rc;
    }
    if ((rc = d2h_finish(ctx))) return rc;
    for (size_t b = 0; b < batch; b++) {
        if (status) status[b] = st[b];
        if (st[b]) rc = BZH_E_RANGE;
    }
    return rc;
}

// What bzh_expr_eval_batch and bzh_vm2_eval put on the device around their launch: the columns (host columns only), the
// constants, the program, the column pointer and stride tables, and room for a host caller's output.
struct ExprStaged {
    Stager s;
    uint32_t *d_consts, *d_prog, *d_ptrs, *d_strides, *d_out;
};
static int stage_expr(bzh_ctx* ctx, int field, int form, int mem, const void* prog, size_t prog_bytes, const uint64_t* const* columns,
                      const size_t* column_strides, size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride,
                      size_t size, size_t batch, uint64_t* out, ExprStaged& st) {
    int rc = BZH_OK;
    if (mem == BZH_MEM_DEVICE && form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
    // host columns: vector v of column c is columns[c] + v * stride * 4 limbs; they are staged as `reps` consecutive copies
    std::vector<size_t> strides(ncols, 0), reps(ncols, 1);
    size_t host_elems = 0;
    for (size_t c = 0; c < ncols; c++) {
        strides[c] = (column_strides && batch > 1) ? column_strides[c] : 0;
        if (strides[c] && strides[c] < size) return BZH_E_ARG;
        reps[c] = strides[c] ? batch : 1;
        host_elems += reps[c] * size;
    }
    const size_t nconst_total = const_stride ? const_stride * (batch - 1) + nconsts : nconsts;
    Stager& s = st.s;
    s = Stager{ctx, field, form};
    if ((rc = s.begin(((mem == BZH_MEM_HOST ? host_elems + batch * size : 0) + nconst_total) * 32 + prog_bytes +
                      ncols * (sizeof(void*) + sizeof(size_t) + 128) + 1024)))
        return rc;
    std::vector<const uint32_t*> ptrs(ncols);
    for (size_t c = 0; c < ncols; c++) {
        if (mem == BZH_MEM_HOST) {
            uint32_t* d = s.carve(reps[c] * size * 32);
            for (size_t v = 0; v < reps[c]; v++)
                BZH_HIP_TRY(ctx, hipMemcpyAsync(d + v * size * 8, columns[c] + v * strides[c] * 4, size * 32, hipMemcpyHostToDevice,
                                                ctx->stream));
            if (form == BZH_FORM_CANONICAL && (rc = field_convert(ctx, field, d, reps[c] * size, 1))) return rc;
            ptrs[c] = d;
            if (strides[c]) strides[c] = size;
        } else {
            ptrs[c] = (const uint32_t*)columns[c];
        }
    }
    if ((rc = s.in(consts, nconst_total, &st.d_consts))) return rc;
    st.d_prog = s.carve(prog_bytes);
    st.d_ptrs = s.carve(ncols * sizeof(void*) + 8);
    st.d_strides = s.carve(ncols * sizeof(size_t) + 8);
    if ((rc = h2d_small(ctx, st.d_prog, prog, prog_bytes))) return rc;
    if (ncols && (rc = h2d_small(ctx, st.d_ptrs, ptrs.data(), ncols * sizeof(void*)))) return rc;
    if (ncols && (rc = h2d_small(ctx, st.d_strides, strides.data(), ncols * sizeof(size_t)))) return rc;
    st.d_out = mem == BZH_MEM_HOST ? s.carve(batch * size * 32) : (uint32_t*)out;
    return BZH_OK;
}

int bzh_expr_eval_batch(bzh_ctx* ctx, int field, const bzh_expr_op* prog, size_t nops, const uint64_t* const* columns,
                        const size_t* column_strides, size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride,
                        unsigned log_size, int result_slot, size_t batch, int form, int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE(!prog || !nops || (!columns && ncols) || (!consts && nconsts) || !out || log_size > 30 ||
                      result_slot < 0 || result_slot >= BZH_EXPR_MAX_SLOTS || !batch || batch > 65535 ||
                      (const_stride && const_stride < nconsts));
    const size_t size = (size_t)1 << log_size;
    int nslots = result_slot + 1;
    for (size_t i = 0; i < nops; i++) {  // validate the program: it indexes device memory
        const bzh_expr_op& o = prog[i];
        if (o.op > BZH_EXPR_COPY || o.dst >= BZH_EXPR_MAX_SLOTS) return BZH_E_ARG;
        nslots = std::max(nslots, (int)o.dst + 1);
        const int kinds[2] = {o.a_kind, (o.op == BZH_EXPR_NEG || o.op == BZH_EXPR_COPY) ? BZH_EXPR_SLOT : o.b_kind};
        const int idxs[2] = {o.a_idx, (o.op == BZH_EXPR_NEG || o.op == BZH_EXPR_COPY) ? 0 : o.b_idx};
        for (int q = 0; q < 2; q++) {
            if (kinds[q] == BZH_EXPR_SLOT && (idxs[q] < 0 || idxs[q] >= BZH_EXPR_MAX_SLOTS)) return BZH_E_ARG;
            if (kinds[q] == BZH_EXPR_SLOT) nslots = std::max(nslots, idxs[q] + 1);
            if (kinds[q] == BZH_EXPR_COLUMN && (idxs[q] < 0 || (size_t)idxs[q] >= ncols)) return BZH_E_ARG;
            if (kinds[q] == BZH_EXPR_CONST && (idxs[q] < 0 || (size_t)idxs[q] >= nconsts)) return BZH_E_ARG;
            if (kinds[q] > BZH_EXPR_CONST || kinds[q] < 0) return BZH_E_ARG;
        }
    }
    ExprStaged st;
    if ((rc = stage_expr(ctx, field, form, mem, prog, nops * sizeof(bzh_expr_op), columns, column_strides, ncols, consts, nconsts,
                         const_stride, size, batch, out, st)))
        return rc;
    rc = expr_eval(ctx, field, st.d_prog, (int)nops, (const uint32_t* const*)st.d_ptrs, (const size_t*)st.d_strides, st.d_consts,
                   const_stride, size, result_slot, batch, nslots, st.d_out);
    if (rc) return rc;
    if (mem == BZH_MEM_HOST) return st.s.out(out, st.d_out, batch * size);
    return BZH_OK;  // staging reuse by the next call is stream-ordered
}

int bzh_expr_eval(bzh_ctx* ctx, int field, const bzh_expr_op* prog, size_t nops, const uint64_t* const* columns, size_t ncols,
                  const uint64_t* consts, size_t nconsts, unsigned log_size, int result_slot, int form, int mem, uint64_t* out) {
    return bzh_expr_eval_batch(ctx, field, prog, nops, columns, nullptr, ncols, consts, nconsts, 0, log_size, result_slot, 1, form, mem,
                               out);
}

// is `o` one of the interpreter's 52 cases, and does everything it indexes exist?  (k_expr_vm2's switch skips a word it has no
// case for, and nothing on the device checks an index)
static bool vm2_op_valid(const ExprOp2& o, size_t ncols, size_t nconsts, int nlds) {
    if (o.code >> 6) return false;
    if (o.form() == V2_SS ? o.pos() > 2 : (o.form() == V2_LL || o.form() == V2_UN) && o.op() == 3) return false;
    auto leaf_ok = [&](int kind, int32_t idx) {
        if (idx < 0) return false;
        switch (kind) {
            case BZH_EXPR_COLUMN: return (size_t)idx < ncols;
            case BZH_EXPR_CONST: return (size_t)idx < nconsts;
            case BZH_EXPR_LDS: return idx < nlds;
        }
        return false;
    };
    if (o.reads_a() && !leaf_ok(o.a_kind, o.a_idx)) return false;
    if (o.reads_b() && !leaf_ok(o.b_kind, o.b_idx)) return false;
    if (o.is_store() && !leaf_ok(BZH_EXPR_LDS, o.a_idx)) return false;
    return true;
}

int bzh_vm2_eval(bzh_ctx* ctx, int field, const void* ops, size_t nops, const uint64_t* const* columns, const size_t* column_strides,
                 size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride, unsigned log_size, size_t batch, int nlds,
                 int form, int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE((field != BZH_FIELD_FP && field != BZH_FIELD_FQ) || !ops || !nops || nops > (size_t)INT32_MAX ||
                      (!columns && ncols) || (!consts && nconsts) || !out || log_size > 30 || !batch || batch > 65535 || nlds < 0 ||
                      (const_stride && const_stride < nconsts));
    const size_t size = (size_t)1 << log_size;
    if (size % 128) return BZH_E_ARG;   // whole workgroups of either kernel
    const ExprOp2* prog = (const ExprOp2*)ops;
    for (size_t i = 0; i < nops; i++)
        if (!vm2_op_valid(prog[i], ncols, nconsts, nlds)) return BZH_E_ARG;
    ExprStaged st;
    if ((rc = stage_expr(ctx, field, form, mem, ops, nops * sizeof(ExprOp2), columns, column_strides, ncols, consts, nconsts, const_stride,
                         size, batch, out, st)))
        return rc;
    rc = expr_eval2(ctx, field, st.d_prog, (int)nops, (const uint32_t* const*)st.d_ptrs, (const size_t*)st.d_strides, st.d_consts,
                    const_stride, size, batch, nlds, st.d_out);
    if (rc) return rc;
    if (mem == BZH_MEM_HOST) return st.s.out(out, st.d_out, batch * size);
    return BZH_OK;  // staging reuse by the next call is stream-ordered
}

// The same program coset by coset (k_expr_vm2_cosets): see include/bzh2.h for the layout of an n-sized column
int bzh_vm2_eval_cosets(bzh_ctx* ctx, int field, const void* ops, size_t nops, const uint64_t* const* columns, const size_t* column_strides,
                        const uint8_t* column_extended, size_t ncols, const uint64_t* consts, size_t nconsts, size_t const_stride,
                        unsigned log_n, size_t out_size, size_t batch, int nlds, int form, int mem, uint64_t* out) {
    BZH_POLY_PROLOGUE((field != BZH_FIELD_FP && field != BZH_FIELD_FQ) || !ops || !nops || nops > (size_t)INT32_MAX ||
                      (!columns && ncols) || (!column_extended && ncols) || (!consts && nconsts) || !out || log_n > 27 || !batch ||
                      batch > 65535 || nlds < 0 || (const_stride && const_stride < nconsts));
    const size_t n = (size_t)1 << log_n, en = n * 8;
    if (out_size != en) return BZH_E_ARG;
    // 8-byte limbs in host memory; whole 32-byte elements in device memory (the kernels load and store them as 16-byte halves)
    const uintptr_t align = mem == BZH_MEM_DEVICE ? 31 : 7;
    uintptr_t all = (uintptr_t)out | (mem == BZH_MEM_HOST ? (uintptr_t)consts : 0);
    for (size_t c = 0; c < ncols; c++) all |= (uintptr_t)columns[c];
    if (all & align) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
    const ExprOp2* prog = (const ExprOp2*)ops;
    for (size_t i = 0; i < nops; i++) {
        if (!vm2_op_valid(prog[i], ncols, nconsts, nlds)) return BZH_E_ARG;
        // a rotation is a step on the extended domain: only a multiple of 8 stays on the lane's coset
        if (prog[i].reads_a() && prog[i].a_kind == BZH_EXPR_COLUMN && prog[i].a_rot % 8) return BZH_E_ARG;
        if (prog[i].reads_b() && prog[i].b_kind == BZH_EXPR_COLUMN && prog[i].b_rot % 8) return BZH_E_ARG;
    }
    // column c, vector v: an extended column at columns[c] + v * stride (8 n elements); an n-sized one as eight blocks, coset j's
    // at columns[c] + j * block, block = batch * stride (or n when shared), vector v at + v * stride
    std::vector<size_t> strides(ncols, 0), reps(ncols, 1), rows(ncols, 0), block(ncols, 0);
    std::vector<uint32_t> shifts(ncols, 0);
    size_t host_elems = 0;
    for (size_t c = 0; c < ncols; c++) {
        rows[c] = column_extended[c] ? en : n;
        shifts[c] = column_extended[c] ? 0u : 3u;
        strides[c] = (column_strides && batch > 1) ? column_strides[c] : 0;
        if (strides[c] && strides[c] < rows[c]) return BZH_E_ARG;
        reps[c] = strides[c] ? batch : 1;
        block[c] = strides[c] ? batch * strides[c] : n;
        host_elems += reps[c] * en;
    }
    const size_t nconst_total = const_stride ? const_stride * (batch - 1) + nconsts : nconsts;
    Stager s{ctx, field, form};
    if ((rc = s.begin(((mem == BZH_MEM_HOST ? host_elems + batch * en : 0) + nconst_total) * 32 + nops * sizeof(ExprOp2) +
                      ncols * (8 * sizeof(void*) + sizeof(size_t) + 4 + 64 * 11) + 2048)))
        return rc;
    std::vector<const uint32_t*> ptrs(8 * ncols);   // [coset][column]
    for (size_t c = 0; c < ncols; c++) {
        const uint32_t* base = (const uint32_t*)columns[c];
        if (mem == BZH_MEM_HOST) {   // staged densely: extended (reps, 8 n) | n-sized (8, reps, n)
            uint32_t* d = s.carve(reps[c] * en * 32);
            const size_t pieces = column_extended[c] ? 1 : 8;
            for (size_t j = 0; j < pieces; j++)
                for (size_t v = 0; v < reps[c]; v++)
                    BZH_HIP_TRY(ctx, hipMemcpyAsync(d + (j * reps[c] + v) * rows[c] * 8, columns[c] + (j * block[c] + v * strides[c]) * 4,
                                                    rows[c] * 32, hipMemcpyHostToDevice, ctx->stream));
            if (form == BZH_FORM_CANONICAL && (rc = field_convert(ctx, field, d, reps[c] * en, 1))) return rc;
            base = d;
            if (strides[c]) strides[c] = rows[c];
            block[c] = reps[c] * n;
        }
        for (size_t j = 0; j < 8; j++) ptrs[j * ncols + c] = column_extended[c] ? base : base + j * block[c] * 8;
    }
    uint32_t *d_consts = nullptr, *d_prog = s.carve(nops * sizeof(ExprOp2)), *d_ptrs[8], *d_strides = s.carve(ncols * sizeof(size_t) + 8),
             *d_shifts = s.carve(ncols * 4 + 8);
    for (size_t j = 0; j < 8; j++) d_ptrs[j] = s.carve(ncols * sizeof(void*) + 8);
    if ((rc = s.in(consts, nconst_total, &d_consts))) return rc;
    if ((rc = h2d_small(ctx, d_prog, ops, nops * sizeof(ExprOp2)))) return rc;
    if (ncols) {
        if ((rc = h2d_small(ctx, d_strides, strides.data(), ncols * sizeof(size_t)))) return rc;
        if ((rc = h2d_small(ctx, d_shifts, shifts.data(), ncols * 4))) return rc;
        for (size_t j = 0; j < 8; j++)
            if ((rc = h2d_small(ctx, d_ptrs[j], ptrs.data() + j * ncols, ncols * sizeof(void*)))) return rc;
    }
    uint32_t* d_out = mem == BZH_MEM_HOST ? s.carve(batch * en * 32) : (uint32_t*)out;
    const uint32_t* const* tables[8];
    for (size_t j = 0; j < 8; j++) tables[j] = (const uint32_t* const*)d_ptrs[j];
    rc = expr_eval2_cosets(ctx, field, d_prog, (int)nops, tables, (const size_t*)d_strides, d_shifts, d_consts, const_stride, log_n, batch,
                           nlds, d_out, nullptr);
    if (rc) return rc;
    if (mem == BZH_MEM_HOST) return s.out(out, d_out, batch * en);
    return BZH_OK;  // staging reuse by the next call is stream-ordered
}

int bzh_ipa_open_batch(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* polys, int form, int mem, size_t batch,
                       const uint64_t* blinds, const uint64_t* x3s, const uint8_t* rng, size_t rng_stride,
                       bzh_transcript* const* transcripts, uint64_t* out_v) {
    if (!ctx || !bases || !polys || !blinds || !x3s || !rng || !transcripts || !out_v || !valid_form(form) || !valid_mem(mem))
        return BZH_E_ARG;
    if (bases->n < 3 || bases->device != ctx->device || !batch || batch > 32767) return BZH_E_ARG;
    const size_t n = bases->n - 2;
    if (n & (n - 1)) return BZH_E_ARG;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    if (rng_stride < 64 * (n + 1 + 2 * (size_t)k)) return BZH_E_ARG;
    for (size_t b = 0; b < batch; b++)
        if (!transcripts[b]) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int field = 0;
    BZH_TRY(with_curve(bases->curve, [&](auto c) {
        field = CurveInfo<decltype(c)>::scalar_field;
        return BZH_OK;
    }));
    if (mem == BZH_MEM_DEVICE) {
        if (form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return ipa_open(ctx, bases, (const uint32_t*)polys, batch, blinds, x3s, rng, rng_stride, transcripts, out_v);
    }
    int rc;
    Stager s{ctx, field, form};  // WS_STAGE; the opening itself works in WS_SCRATCH_*, WS_IPA and WS_IPA_OUT
    if ((rc = s.begin(batch * n * 32))) return rc;
    uint32_t* d_polys;
    if ((rc = s.in(polys, batch * n, &d_polys))) return rc;
    return ipa_open(ctx, bases, d_polys, batch, blinds, x3s, rng, rng_stride, transcripts, out_v);
}

int bzh_ipa_open_batch_device(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* polys, int form, int mem, size_t batch,
                              const uint64_t* blinds, const uint64_t* x3s, const uint8_t* rng, size_t rng_stride,
                              bzh_transcript_batch* transcripts, uint64_t* out_v, uint8_t* status) {
    if (!ctx || !bases || !polys || !blinds || !x3s || !rng || !transcripts || !out_v || !valid_form(form) || !valid_mem(mem))
        return BZH_E_ARG;
    if (bases->n < 3 || bases->device != ctx->device || !batch || batch > 65535) return BZH_E_ARG;
    const size_t n = bases->n - 2;
    if (n & (n - 1)) return BZH_E_ARG;
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    const size_t nrand = n + 1 + 2 * (size_t)k;
    if (rng_stride < 64 * nrand) return BZH_E_ARG;
    const TbInfo ti = tb_info(transcripts);
    if (ti.ctx != ctx || ti.curve != bases->curve || ti.batch != batch) return BZH_E_ARG;   // (a host-resident batch has no ctx)
    if (mem == BZH_MEM_DEVICE &&
        (((uintptr_t)polys | (uintptr_t)blinds | (uintptr_t)x3s | (uintptr_t)rng | (uintptr_t)out_v) & 15))
        return BZH_E_ARG;
    if (ti.proof_len + 32 * (1 + 2 * (size_t)k) + 64 > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int field = 0;
    BZH_TRY(with_curve(bases->curve, [&](auto c) {
        field = CurveInfo<decltype(c)>::scalar_field;
        return BZH_OK;
    }));
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const size_t st_bytes = (batch + 15) & ~(size_t)15;
    // WS_STAGE (the opening itself works in WS_SCRATCH_*, WS_IPA and WS_IPA_OUT): host operands are staged up here once, and canonical
    // coefficients get their Montgomery copy here
    Stager s{ctx, field, form};
    BZH_TRY(s.begin(((host || canonical) ? batch * n * 32 + 64 : 0) + (host ? batch * (96 + nrand * 64) + st_bytes + 5 * 64 : 0)));
    const uint32_t* d_polys = (const uint32_t*)polys;
    if (host) {
        uint32_t* d = nullptr;
        BZH_TRY(s.in(polys, batch * n, &d));
        d_polys = d;
    } else if (canonical) {
        uint32_t* d = s.carve(batch * n * 32);
        BZH_HIP_TRY(ctx, hipMemcpyAsync(d, polys, batch * n * 32, hipMemcpyDeviceToDevice, ctx->stream));
        BZH_TRY(field_convert(ctx, field, d, batch * n, 1));
        d_polys = d;
    }
    if (!host)
        return ipa_open_device(ctx, bases, d_polys, batch, (const uint32_t*)blinds, (const uint32_t*)x3s, form, rng, rng_stride, transcripts,
                               (uint32_t*)out_v, status);
    uint32_t *d_blinds = s.carve(batch * 32), *d_x3s = s.carve(batch * 32), *d_v = s.carve(batch * 32);
    uint8_t* d_rng = (uint8_t*)s.carve(batch * nrand * 64);
    uint8_t* d_st = (uint8_t*)s.carve(st_bytes);
    BZH_TRY(h2d_small(ctx, d_blinds, blinds, batch * 32));
    BZH_TRY(h2d_small(ctx, d_x3s, x3s, batch * 32));
    for (size_t b = 0; b < batch; b++) BZH_TRY(h2d_small(ctx, d_rng + b * nrand * 64, rng + b * rng_stride, nrand * 64));
    BZH_TRY(ipa_open_device(ctx, bases, d_polys, batch, d_blinds, d_x3s, form, d_rng, nrand * 64, transcripts, d_v, d_st));
    std::vector<uint8_t> st(st_bytes);
    BZH_TRY(d2h_async(ctx, out_v, d_v, batch * 32));
    BZH_TRY(d2h_async(ctx, st.data(), d_st, st_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (status) memcpy(status, st.data(), batch);
    return BZH_OK;
}

int bzh_multiopen_batch_device(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, unsigned k, const uint64_t* polys, size_t npolys_own,
                               const uint64_t* shared, size_t npolys_shared, const uint64_t* blinds, const uint64_t* shared_blinds,
                               const uint64_t* points, size_t npoints, const bzh_open_query* queries, size_t nqueries, int form, int mem,
                               const uint8_t* rng, size_t rng_stride, bzh_transcript_batch* transcripts, uint8_t* status) {
    if (!ctx || !bases || !transcripts || !polys || !blinds || !points || !queries || !rng || !valid_form(form) || !valid_mem(mem))
        return BZH_E_ARG;
    if (!npolys_own || (npolys_shared && (!shared || !shared_blinds)) || !batch || batch > 65535 || k > 31) return BZH_E_ARG;
    const size_t n = (size_t)1 << k, npolys = npolys_own + npolys_shared, nrand = n + 2 + 2 * (size_t)k;
    if (rng_stride < 64 * nrand) return BZH_E_ARG;
    MoPlan plan;
    plan.npolys_own = npolys_own, plan.npolys_shared = npolys_shared, plan.npoints = npoints;
    plan.set_of_poly.resize(npolys), plan.group_order.resize(npolys), plan.set_sizes.resize(npolys);
    plan.set_points.resize(npolys * BZH_MULTIOPEN_MAX_POINTS);
    BZH_TRY(bzh_multiopen_plan(queries, nqueries, npolys, npoints, plan.set_of_poly.data(), plan.group_order.data(), plan.set_sizes.data(),
                               plan.set_points.data(), &plan.nsets));
    for (size_t s = 0; s < plan.nsets; s++)
        if (plan.set_sizes[s] >= n) return BZH_E_ARG;   // nothing is left of n coefficients after n divisions
    const TbInfo ti = tb_info(transcripts);
    if (ti.ctx != ctx || ti.batch != batch) return BZH_E_ARG;   // (a host-resident batch has no ctx)
    if (bases->n != n + 2 || bases->device != ctx->device || ti.curve != bases->curve) return BZH_E_ARG;
    const uintptr_t all = (uintptr_t)polys | (uintptr_t)shared | (uintptr_t)blinds | (uintptr_t)shared_blinds | (uintptr_t)points | (uintptr_t)rng;
    if (mem == BZH_MEM_DEVICE && (all & 15)) return BZH_E_ARG;
    if (ti.proof_len + 32 + 32 * plan.nsets + 32 * (1 + 2 * (size_t)k) + 64 > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int field = 0;
    BZH_TRY(with_curve(bases->curve, [&](auto c) {
        field = CurveInfo<decltype(c)>::scalar_field;
        return BZH_OK;
    }));
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const size_t st_bytes = (batch + 15) & ~(size_t)15, own = batch * npolys_own * n, shr = npolys_shared * n;
    // the staging workspace holds, side by side: the polynomials' Montgomery copy (host or canonical operands), the small host
    // operands, and the call's own scratch
    Stager s{ctx, field, form};
    BZH_TRY(s.begin(((host || canonical) ? (own + shr) * 32 + 128 : 0) +
                    (host ? (batch * (npolys_own + npoints) + npolys_shared) * 32 + batch * nrand * 64 + st_bytes + 5 * 64 : 0) +
                    multiopen_scratch_bytes(plan, batch, n) + 64));
    const uint32_t *d_polys = (const uint32_t*)polys, *d_shared = (const uint32_t*)shared;
    auto montgomery_copy = [&](const uint64_t* src, size_t elems, const uint32_t** dev) -> int {
        uint32_t* d = nullptr;
        if (host) {
            BZH_TRY(s.in(src, elems, &d));
        } else {
            d = s.carve(elems * 32);
            BZH_HIP_TRY(ctx, hipMemcpyAsync(d, src, elems * 32, hipMemcpyDeviceToDevice, ctx->stream));
            BZH_TRY(field_convert(ctx, field, d, elems, 1));
        }
        *dev = d;
        return BZH_OK;
    };
    if (host || canonical) {
        BZH_TRY(montgomery_copy(polys, own, &d_polys));
        if (shr) BZH_TRY(montgomery_copy(shared, shr, &d_shared));
    }
    if (!host)
        return multiopen_device(ctx, bases, batch, k, plan, d_polys, d_shared, (const uint32_t*)blinds, (const uint32_t*)shared_blinds,
                                (const uint32_t*)points, form, rng, rng_stride, transcripts, status, s.carve(0));
    uint32_t *d_blinds = s.carve(batch * npolys_own * 32), *d_sblinds = s.carve(npolys_shared * 32), *d_points = s.carve(batch * npoints * 32);
    uint8_t* d_rng = (uint8_t*)s.carve(batch * nrand * 64);
    uint8_t* d_st = (uint8_t*)s.carve(st_bytes);
    BZH_TRY(h2d_small(ctx, d_blinds, blinds, batch * npolys_own * 32));
    BZH_TRY(h2d_small(ctx, d_sblinds, shared_blinds, npolys_shared * 32));
    BZH_TRY(h2d_small(ctx, d_points, points, batch * npoints * 32));
    for (size_t b = 0; b < batch; b++) BZH_TRY(h2d_small(ctx, d_rng + b * nrand * 64, rng + b * rng_stride, nrand * 64));
    BZH_TRY(multiopen_device(ctx, bases, batch, k, plan, d_polys, d_shared, d_blinds, d_sblinds, d_points, form, d_rng, nrand * 64, transcripts,
                             d_st, s.carve(0)));
    std::vector<uint8_t> st(st_bytes);
    BZH_TRY(d2h_async(ctx, st.data(), d_st, st_bytes));
    BZH_TRY(d2h_finish(ctx));
    if (status) memcpy(status, st.data(), batch);
    return BZH_OK;
}

int bzh_evaluations_batch_device(bzh_ctx* ctx, size_t batch, unsigned k, const uint64_t* polys, size_t npolys_own, const uint64_t* shared,
                                 size_t npolys_shared, const bzh_eval_query* queries, size_t nqueries, const uint64_t* h_pieces,
                                 size_t npieces, size_t h_stride, const uint64_t* h_blinds, int form, int mem,
                                 bzh_transcript_batch* transcripts, uint64_t* out_points, uint64_t* out_evals, uint64_t* out_h,
                                 uint64_t* out_h_blind) {
    if (!ctx || !transcripts || !polys || !queries || !out_points || !valid_form(form) || !valid_mem(mem)) return BZH_E_ARG;
    if (!npolys_own || (npolys_shared && !shared) || !batch || batch > 65535 || k > 32) return BZH_E_ARG;
    if (npieces && (!h_pieces || !h_blinds || !out_h || !out_h_blind)) return BZH_E_ARG;
    const size_t n = (size_t)1 << k, npolys = npolys_own + npolys_shared;
    if (npieces && (npieces > ((size_t)1 << 20) || h_stride < npieces * n)) return BZH_E_ARG;
    if (!nqueries) return BZH_E_ARG;
    EvPlan plan;
    plan.npolys_own = npolys_own, plan.npolys_shared = npolys_shared, plan.nqueries = nqueries;
    plan.rotations.resize(nqueries), plan.point_of_query.resize(nqueries), plan.poly_order.resize(npolys), plan.rot_count.resize(npolys);
    BZH_TRY(bzh_evaluations_plan(queries, nqueries, npolys, plan.rotations.data(), &plan.nrot, plan.point_of_query.data(),
                                 plan.poly_order.data(), plan.rot_count.data()));
    plan.rotations.resize(plan.nrot);
    plan.poly_of_query.resize(nqueries);
    for (size_t q = 0; q < nqueries; q++) plan.poly_of_query[q] = queries[q].poly;
    const TbInfo ti = tb_info(transcripts);
    if (ti.ctx != ctx || ti.batch != batch) return BZH_E_ARG;   // (a host-resident batch has no ctx)
    int field = 0;
    BZH_TRY(with_curve(ti.curve, [&](auto c) {
        field = CurveInfo<decltype(c)>::scalar_field;
        return BZH_OK;
    }));
    if (k > field_two_adicity(field)) return BZH_E_ARG;
    if (!npieces) h_pieces = h_blinds = nullptr, out_h = out_h_blind = nullptr;
    const uintptr_t all = (uintptr_t)polys | (uintptr_t)shared | (uintptr_t)h_pieces | (uintptr_t)h_blinds | (uintptr_t)out_points |
                          (uintptr_t)out_evals | (uintptr_t)out_h | (uintptr_t)out_h_blind;
    if (mem == BZH_MEM_DEVICE && (all & 15)) return BZH_E_ARG;
    if (ti.proof_len + 32 * nqueries > ti.proof_cap) return BZH_E_RANGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool host = mem == BZH_MEM_HOST, canonical = form == BZH_FORM_CANONICAL;
    const size_t own = batch * npolys_own * n, shr = npolys_shared * n, hrow = npieces * n, nrot = plan.nrot;
    // the staging workspace holds, side by side: the polynomials' and the pieces' Montgomery copy (host or canonical operands), the
    // host call's blinds and outputs, and the call's own scratch
    Stager s{ctx, field, form};
    BZH_TRY(s.begin(((host || canonical) ? (own + shr + batch * hrow) * 32 + 3 * 64 : 0) +
                    (host ? batch * (npieces + nrot + nqueries + n + 1) * 32 + 5 * 64 : 0) + evaluations_scratch_bytes(plan, batch, npieces) + 64));
    const uint32_t *d_polys = (const uint32_t*)polys, *d_shared = (const uint32_t*)shared, *d_h = (const uint32_t*)h_pieces;
    size_t d_h_stride = h_stride;
    // rows of `row` elements, `stride` apart at the caller's, side by side in the workspace and in Montgomery form
    auto montgomery_copy = [&](const uint64_t* src, size_t rows, size_t row, size_t stride, const uint32_t** dev) -> int {
        uint32_t* d = s.carve(rows * row * 32);
        if (stride == row) row *= rows, stride = row, rows = 1;   // one piece
        if (host) {
            for (size_t r = 0; r < rows; r++) BZH_TRY(h2d_small(ctx, d + r * row * 8, src + r * stride * 4, row * 32));
        } else if (rows == 1) {
            BZH_HIP_TRY(ctx, hipMemcpyAsync(d, src, row * 32, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            BZH_HIP_TRY(ctx, hipMemcpy2DAsync(d, row * 32, src, stride * 32, row * 32, rows, hipMemcpyDeviceToDevice, ctx->stream));
        }
        *dev = d;
        return BZH_OK;
    };
    if (host || canonical) {
        BZH_TRY(montgomery_copy(polys, batch, npolys_own * n, npolys_own * n, &d_polys));
        if (shr) BZH_TRY(montgomery_copy(shared, 1, shr, shr, &d_shared));
        if (npieces) BZH_TRY(montgomery_copy(h_pieces, batch, hrow, h_stride, &d_h));
        d_h_stride = hrow;
        if (canonical) {   // the three copies lie side by side, 64-byte aligned: one conversion each
            BZH_TRY(field_convert(ctx, field, (uint32_t*)d_polys, own, 1));
            if (shr) BZH_TRY(field_convert(ctx, field, (uint32_t*)d_shared, shr, 1));
            if (npieces) BZH_TRY(field_convert(ctx, field, (uint32_t*)d_h, batch * hrow, 1));
        }
    }
    if (!host) {
        BZH_TRY(evaluations_device(ctx, ti.curve, batch, k, plan, d_polys, d_shared, d_h, npieces, d_h_stride, (const uint32_t*)h_blinds, form,
                                   transcripts, (uint32_t*)out_points, (uint32_t*)out_evals, (uint32_t*)out_h, (uint32_t*)out_h_blind,
                                   s.carve(0)));
        if (npieces && canonical) BZH_TRY(field_convert(ctx, field, (uint32_t*)out_h, batch * n, 0));
        return BZH_OK;
    }
    uint32_t *d_hbl = s.carve(batch * npieces * 32), *d_pts = s.carve(batch * nrot * 32), *d_ev = s.carve(batch * nqueries * 32);
    uint32_t *d_oh = s.carve(npieces ? batch * n * 32 : 0), *d_ohb = s.carve(batch * 32);
    if (npieces) BZH_TRY(h2d_small(ctx, d_hbl, h_blinds, batch * npieces * 32));
    BZH_TRY(evaluations_device(ctx, ti.curve, batch, k, plan, d_polys, d_shared, d_h, npieces, d_h_stride, d_hbl, form, transcripts, d_pts, d_ev,
                               d_oh, d_ohb, s.carve(0)));
    BZH_TRY(d2h_async(ctx, out_points, d_pts, batch * nrot * 32));
    if (out_evals) BZH_TRY(d2h_async(ctx, out_evals, d_ev, batch * nqueries * 32));
    if (npieces) {
        if (canonical) BZH_TRY(field_convert(ctx, field, d_oh, batch * n, 0));
        BZH_TRY(d2h_async(ctx, out_h, d_oh, batch * n * 32));
        BZH_TRY(d2h_async(ctx, out_h_blind, d_ohb, batch * 32));
    }
    return d2h_finish(ctx);
}

int bzh_ipa_open(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* poly, int form, int mem, const uint64_t* blind,
                 const uint64_t* x3, const uint8_t* rng, size_t rng_len, bzh_transcript* transcript, uint64_t* out_v) {
    return bzh_ipa_open_batch(ctx, bases, poly, form, mem, 1, blind, x3, rng, rng_len, &transcript, out_v);
}

int bzh_ipa_verify(bzh_ctx* ctx, const bzh_bases* bases, const uint64_t* commitment_xy, const uint64_t* x3, const uint64_t* v,
                   const uint8_t* proof, size_t proof_len, bzh_transcript* transcript, const uint64_t* g0_u_w) {
    if (!ctx || !bases || !commitment_xy || !x3 || !v || !proof || !transcript || !g0_u_w) return BZH_E_ARG;
    if (bases->n < 3 || bases->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ipa_verify(ctx, bases, commitment_xy, x3, v, proof, proof_len, transcript, g0_u_w);
}

int bzh_ipa_check_accumulated(bzh_ctx* ctx, const bzh_bases* bases, size_t batch, size_t nl, const uint64_t* lc_pts, const uint64_t* lc_scal,
                              const uint64_t* cu, const uint64_t* weights, const uint8_t* exclude, int* ok) {
    if (!ctx || !bases || !batch || batch > 4096 || !nl || nl > 65536 || !lc_pts || !lc_scal || !cu || !weights || !ok) return BZH_E_ARG;
    if (bases->n < 3 || bases->device != ctx->device) return BZH_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ipa_check_accumulated(ctx, bases, batch, nl, lc_pts, lc_scal, cu, weights, exclude, ok);
}

int bzh_jacobian_to_affine(int curve, const uint64_t* xyz, size_t n, int form, uint64_t* out_xy) {
    if ((!xyz || !out_xy) && n) return BZH_E_ARG;
    if (!valid_curve(curve) || !valid_form(form)) return BZH_E_ARG;
    return with_curve(curve, [&](auto c) {
        h_jac_to_affine<typename decltype(c)::Base>(xyz, n, form, form, out_xy);
        return BZH_OK;
    });
}

int bzh_jacobian_sum(int curve, const uint64_t* xyz, size_t n, int form, uint64_t* out_xyz) {
    if (!out_xyz || (!xyz && n)) return BZH_E_ARG;
    if (!valid_curve(curve) || !valid_form(form)) return BZH_E_ARG;
    return with_curve(curve, [&](auto c) {
        jac_sum_host<typename decltype(c)::Base>(xyz, n, form, out_xyz);
        return BZH_OK;
    });
}

int bzh_affine_compress(int curve, const uint64_t* xy, size_t n, int form, uint8_t* out32) {
    if ((!xy || !out32) && n) return BZH_E_ARG;
    if (!valid_curve(curve) || !valid_form(form)) return BZH_E_ARG;
    return with_curve(curve, [&](auto c) {
        for (size_t i = 0; i < n; i++) h_compress<decltype(c)>(xy + 8 * i, form, out32 + 32 * i);
        return BZH_OK;
    });
}

int bzh_field_omega(int field, unsigned log_n, int form, uint64_t* out) {
    if (!out || !valid_field(field) || !valid_form(form)) return BZH_E_ARG;
    if (log_n > field_two_adicity(field)) return BZH_E_RANGE;
    return with_field(field, [&](auto p) {
        fe_to_u64(out, h_omega<decltype(p)>(log_n), form);
        return BZH_OK;
    });
}

}  // extern "C"
