// C ABI of the circuit front end (include/bzh2.h, "circuits"): the reference's ShotCircuit / BoardCircuit as
// constraint-system DATA for bzh_pk_create, and their witness synthesis for bzh_prove_batch.
//
// Replaces, on the reference side, `Circuit::configure` + the keygen `synthesize` (keygen_vk / keygen_pk:
// benches/shot.rs:60-61, benches/board.rs:53-54) and the `synthesize` call-back create_proof makes per proof
// (src/circuits/shot.rs:40-52 -> src/chips/shot.rs:308-354; src/circuits/board.rs:38-50 ->
// src/chips/board.rs:331-363).  Chips live in csrc/circuit/*.hpp (host C++); the only device code here is the kernel
// that expands the compact staged witness into the advice tensor.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>

#include "blake2b.hpp"
#include "pedersen_generators.hpp"
#include "circuit/chips.hpp"
#include "ctx.hpp"
#include "synthesize_device.hpp"

using namespace bzc;

namespace {

// GENERATOR constants of the two fixed bases: hash_to_curve("battlezips:hash2curve")(b"v" / b"r") on Pallas
// (src/utils/constants/fixed_bases/board_commit_v.rs:5-14, board_commit_r.rs:5-14; their `generator` tests :2941-2948)
static const uint64_t* const GEN_V = bzh::PEDERSEN_GEN_V;
static const uint64_t* const GEN_R = bzh::PEDERSEN_GEN_R;

static Aff aff_from_limbs(const uint64_t* l) {
    Fp x, y;
    if (!Fp::from_limbs(l, &x) || !Fp::from_limbs(l + 4, &y)) throw std::logic_error("generator constant");
    return Aff{x, y};
}

// ---- fixed-base tables: derived once per process (Z search), cached on disk next to the library -------------------
// A cached file is re-validated on load against the window points derived from the generator (u^2 = y + z, z - y a
// non-square: the two properties the reference's `z` tests assert, board_commit_{v,r}.rs:2950-2960); that z is the SMALLEST
// such value is what tests/test_params_cpu.py checks against all 170 Z / 1 360 U values of the reference through
// bzh_fixed_base_tables -- the cache is never tracked in git (the build writes it to <library dir>/.bzh2_cache too).
static std::string cache_dir() {
    const char* env = getenv("BZH_CACHE_DIR");
    if (env && *env) return env;
    Dl_info info;
    if (dladdr((void*)&cache_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t s = p.rfind('/');
        return (s == std::string::npos ? std::string(".") : p.substr(0, s)) + "/.bzh2_cache";
    }
    return ".bzh2_cache";
}
static bool load_zu(const std::string& path, const Aff& gen, FixedBase& fb) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const int NW = ECC_NUM_WINDOWS;
    std::vector<uint64_t> buf(8 + NW + (size_t)NW * ECC_H * 4);
    const bool ok = fread(buf.data(), 8, buf.size(), f) == buf.size();
    fclose(f);
    if (!ok) return false;
    uint64_t g[8];
    Fp(gen.x).to_limbs(g);
    Fp(gen.y).to_limbs(g + 4);
    if (memcmp(g, buf.data(), 64) != 0) return false;
    fb.z.assign(buf.begin() + 8, buf.begin() + 8 + NW);
    fb.u.resize(NW);
    for (int w = 0; w < NW; w++) {
        for (int k = 0; k < ECC_H; k++) {
            if (!Fp::from_limbs(&buf[8 + NW + ((size_t)w * ECC_H + k) * 4], &fb.u[w][k])) return false;
            if (fb.u[w][k].sqr() != fb.points[w][k].y + Fp::from_u64(fb.z[w])) return false;   // u^2 = y + z
            if ((Fp::from_u64(fb.z[w]) - fb.points[w][k].y).jacobi() >= 0) return false;        // z - y must not be a square
        }
    }
    return true;
}
static void save_zu(const std::string& dir, const std::string& path, const Aff& gen, const FixedBase& fb) {
    mkdir(dir.c_str(), 0755);
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    std::vector<uint64_t> buf(8);
    Fp(gen.x).to_limbs(buf.data());
    Fp(gen.y).to_limbs(buf.data() + 4);
    buf.insert(buf.end(), fb.z.begin(), fb.z.end());
    for (auto& row : fb.u) {
        for (auto& v : row) {
            uint64_t l[4];
            v.to_limbs(l);
            buf.insert(buf.end(), l, l + 4);
        }
    }
    const bool ok = fwrite(buf.data(), 8, buf.size(), f) == buf.size();
    fclose(f);
    if (ok) {
        rename(tmp.c_str(), path.c_str());
    } else {
        remove(tmp.c_str());
    }
}
static FixedBase cached_fixed_base(const Aff& gen, const char* tag) {
    const std::string dir = cache_dir(), path = dir + "/fixed_base_" + tag + "_v1.bin";
    FixedBase fb;
    fb.generator = gen;
    fixed_base_window_points(gen, ECC_NUM_WINDOWS, fb.points);
    if (load_zu(path, gen, fb)) {
        std::vector<Fp> pts;
        for (int k = 0; k < ECC_H; k++) pts.push_back(Fp::from_u64((uint64_t)k));
        fb.lagrange.resize(ECC_NUM_WINDOWS);
        for (int w = 0; w < ECC_NUM_WINDOWS; w++) {
            std::vector<Fp> xs(ECC_H);
            for (int k = 0; k < ECC_H; k++) xs[k] = fb.points[w][k].x;
            const std::vector<Fp> co = lagrange_interpolate(pts, xs);
            for (int k = 0; k < ECC_H; k++) fb.lagrange[w][k] = co[k];
        }
        return fb;
    }
    fb = make_fixed_base(gen);
    save_zu(dir, path, gen, fb);
    return fb;
}
static const BoardFixedBases& fixed_bases() {
    static std::once_flag once;
    static std::unique_ptr<BoardFixedBases> fb;
    std::call_once(once, [] {
        std::unique_ptr<BoardFixedBases> p(new BoardFixedBases());
        p->v = cached_fixed_base(aff_from_limbs(GEN_V), "v");
        p->r = cached_fixed_base(aff_from_limbs(GEN_R), "r");
        fb = std::move(p);
    });
    return *fb;
}

// test circuits of the reference's bitify unit tests (src/chips/bitify.rs:255-403)
struct BitifyTestConfig {
    BitifyConfig bitify;
    Column bits, lc1, e2, fixed;
};
static BitifyTestConfig bitify_test_configure(ConstraintSystem& meta, bool num2bits) {
    BitifyTestConfig c;
    c.bits = meta.advice_column();
    c.lc1 = meta.advice_column();
    c.e2 = meta.advice_column();
    c.fixed = meta.fixed_column();
    meta.enable_equality(c.bits);
    meta.enable_equality(c.lc1);
    meta.enable_equality(c.e2);
    meta.enable_constant(c.fixed);
    c.bitify = num2bits ? num2bits_configure(meta, c.bits, c.lc1, c.e2, c.fixed) : bits2num_configure(meta, c.bits, c.lc1, c.e2, c.fixed);
    const Column trace = meta.advice_column();
    meta.enable_equality(trace);
    return c;
}

}  // namespace

struct bzh_circuit {
    int kind = 0;
    unsigned k = 0;
    unsigned bits = 0;  // bitify test circuits: B
    ConstraintSystem cs;
    ShotConfig shot;
    BoardConfig board;
    BitifyTestConfig bitify;
    Assembly keygen;                   // fixed columns (selector columns appended), copies, regions
    std::vector<size_t> region_starts;
    size_t rows_used = 0;              // advice rows [0, rows_used) are the only ones synthesis writes
    std::vector<uint8_t> blob;
    std::string describe;
    int num_instance_rows = 0;
    bool vk_placeholder = true;        // the blob's vk_repr field is still BZH_VK_REPR_PLACEHOLDER (bzh_circuit_set_vk_repr not called)
};

namespace {

struct AnyInput {
    ShotInput shot;
    BoardInput board;
    Fp value;          // bitify tests
    BinaryValue binary;
};

// one synthesis pass of the circuit's `synthesize` into `lay`; returns the public inputs (instance column 0)
static std::vector<Fp> run_synthesize(const bzh_circuit& c, Layouter& lay, const AnyInput& in) {
    std::vector<Fp> inst;
    switch (c.kind) {
        case BZH_CIRCUIT_SHOT: {
            const Aff cm = shot_synthesize(c.shot, lay, fixed_bases(), in.shot);
            inst = {cm.x, cm.y, Fp::from_u128(in.shot.shot.lower_u128()), Fp::from_u128(in.shot.hit.lower_u128())};
            break;
        }
        case BZH_CIRCUIT_BOARD: {
            const Aff cm = board_synthesize(c.board, lay, fixed_bases(), in.board);
            inst = {cm.x, cm.y};
            break;
        }
        case BZH_CIRCUIT_NUM2BITS_TEST: {
            const AssignedCell value = lay.assign_region("trace", [&](Region& region) { return region.assign_advice(c.bitify.bits, 0, in.value); });
            std::vector<Fp> bits(c.bits);
            for (unsigned i = 0; i < c.bits; i++) bits[i] = in.binary.bit_fp((int)i);
            num2bits_synthesize(c.bitify.bitify, lay, value, bits);
            break;
        }
        case BZH_CIRCUIT_BITS2NUM_TEST: {
            const std::vector<AssignedCell> assigned = lay.assign_region("trace", [&](Region& region) {
                std::vector<AssignedCell> a;
                for (unsigned i = 0; i < c.bits; i++) a.push_back(region.assign_advice(c.bitify.bits, i, in.binary.bit_fp((int)i)));
                return a;
            });
            bits2num_synthesize(c.bitify.bitify, lay, assigned);
            break;
        }
        default: throw std::logic_error("circuit kind");
    }
    return inst;
}

static AnyInput default_input(int kind) {
    // pattern #1 board, shot (3, 5), hit (src/circuits/shot.rs:102-112, src/circuits/board.rs:101-107)
    AnyInput in;
    Board b;
    b.deck.add(0, 3, 3, true);
    b.deck.add(1, 5, 4, false);
    b.deck.add(2, 0, 1, false);
    b.deck.add(3, 0, 5, true);
    b.deck.add(4, 6, 1, false);
    const int opts[5] = {0, 0, 0, 0, 0};
    in.shot.board = b.state(opts);
    in.shot.trapdoor = Fq::from_u64(0x5eed);
    const uint8_t sx = 3, sy = 5;
    in.shot.shot = serialize_shot(&sx, &sy, 1);
    in.shot.hit = BinaryValue::from_u8(1);
    b.witness(opts, in.board.ship_commitments);
    in.board.board = in.shot.board;
    in.board.trapdoor = in.shot.trapdoor;
    in.value = Fp::zero();
    (void)kind;
    return in;
}

static const char* kind_name(int t) { return t == ADVICE ? "advice" : (t == FIXED ? "fixed" : "instance"); }
static std::string json_escape(const std::string& s) {
    std::string o;
    for (char ch : s) {
        if (ch == '"' || ch == '\\') o.push_back('\\');
        o.push_back(ch);
    }
    return o;
}

static void build_blob_and_describe(bzh_circuit& c) {
    ConstraintSystem& cs = c.cs;
    const size_t n = c.keygen.n;
    BlobWriter w;
    w.u32(0x32435A42u);  // "BZC2"
    w.u32(c.k);
    w.u32((uint32_t)cs.num_advice);
    w.u32((uint32_t)cs.num_fixed);
    w.u32((uint32_t)cs.num_instance);
    w.u32((uint32_t)cs.degree());
    // the verifying-key digest create_proof absorbs first (upstream: vk.hash_into).  It is an INPUT of the boundary
    // (bzh_circuit_set_vk_repr, include/bzh2.h): a placeholder until the caller hands over the reference-side value.
    uint8_t vk_repr[32] = {BZH_VK_REPR_PLACEHOLDER & 0xff, BZH_VK_REPR_PLACEHOLDER >> 8};
    if (w.b.size() != BZH_CIRCUIT_BLOB_VK_REPR_OFFSET) throw std::logic_error("blob header layout");
    w.b.insert(w.b.end(), vk_repr, vk_repr + 32);
    uint32_t npolys = 0;
    for (auto& g : cs.gates) npolys += (uint32_t)g.polys.size();
    w.u32(npolys);
    for (auto& g : cs.gates) {
        for (auto& p : g.polys) w.expr(p);
    }
    w.u32((uint32_t)cs.permutation.size());
    for (auto& pc : cs.permutation) {
        w.u8((uint8_t)pc.kind);
        w.u32((uint32_t)pc.index);
    }
    w.u32((uint32_t)cs.lookups.size());
    for (auto& lk : cs.lookups) {
        w.u32((uint32_t)lk.inputs.size());
        for (auto& e : lk.inputs) w.expr(e);
        for (auto& e : lk.tables) w.expr(e);
    }
    auto perm_index = [&](const Column& col) -> uint32_t {
        for (size_t i = 0; i < cs.permutation.size(); i++) {
            if (cs.permutation[i] == col) return (uint32_t)i;
        }
        throw std::logic_error("copy constraint on a column without equality enabled");
    };
    w.u32((uint32_t)c.keygen.copies.size());
    for (auto& cp : c.keygen.copies) {
        w.u32(perm_index(cp.a));
        w.u32((uint32_t)cp.row_a);
        w.u32(perm_index(cp.b));
        w.u32((uint32_t)cp.row_b);
    }
    for (int f = 0; f < cs.num_fixed; f++) {
        const std::vector<Fp>& col = c.keygen.fixed[f];
        size_t len = n;
        while (len && col[len - 1].is_zero()) len--;
        w.u32((uint32_t)len);
        for (size_t r = 0; r < len; r++) w.fe(col[r]);
    }
    // explicit query lists, in upstream's registration order (enable_equality registers before any gate does)
    for (const std::vector<Query>* qs : {&cs.advice_queries, &cs.fixed_queries, &cs.instance_queries}) {
        w.u32((uint32_t)qs->size());
        for (auto& q : *qs) {
            w.u32((uint32_t)q.column);
            w.u32((uint32_t)q.rotation);
        }
    }
    c.blob.swap(w.b);

    std::ostringstream o;
    o << "{\"kind\":" << c.kind << ",\"k\":" << c.k << ",\"num_advice\":" << cs.num_advice << ",\"num_fixed\":" << cs.num_fixed
      << ",\"num_instance\":" << cs.num_instance << ",\"num_selectors\":" << cs.num_selectors << ",\"degree\":" << cs.degree()
      << ",\"blinding_factors\":" << cs.blinding_factors() << ",\"usable_rows\":" << c.keygen.usable_rows << ",\"rows_used\":" << c.rows_used
      << ",\"num_polys\":" << npolys << ",\"num_copies\":" << c.keygen.copies.size() << ",\"gates\":[";
    uint32_t first = 0;
    for (size_t gi = 0; gi < cs.gates.size(); gi++) {
        const Gate& g = cs.gates[gi];
        o << (gi ? "," : "") << "{\"name\":\"" << json_escape(g.name) << "\",\"first_poly\":" << first << ",\"constraints\":[";
        for (size_t i = 0; i < g.constraint_names.size(); i++) o << (i ? "," : "") << "\"" << json_escape(g.constraint_names[i]) << "\"";
        o << "],\"queried_cells\":[";
        for (size_t i = 0; i < g.queried_cells.size(); i++)
            o << (i ? "," : "") << "[\"" << kind_name(g.queried_cells[i].kind) << "\"," << g.queried_cells[i].column << "," << g.queried_cells[i].rotation << "]";
        o << "]}";
        first += (uint32_t)g.polys.size();
    }
    o << "],\"regions\":[";
    for (size_t ri = 0; ri < c.keygen.regions.size(); ri++) {
        const RegionInfo& r = c.keygen.regions[ri];
        o << (ri ? "," : "") << "{\"name\":\"" << json_escape(r.name) << "\",\"has_rows\":" << (r.has_rows ? "true" : "false") << ",\"row_lo\":" << r.row_lo
          << ",\"row_hi\":" << r.row_hi << ",\"columns\":[";
        size_t i = 0;
        for (auto& col : r.columns) o << (i++ ? "," : "") << "[\"" << kind_name(col.kind) << "\"," << col.index << "]";
        o << "],\"advice_cells\":[";   // every advice cell the region assigns: (column, absolute row)
        i = 0;
        for (auto& ac : r.advice_cells) o << (i++ ? "," : "") << "[" << ac.first << "," << ac.second << "]";
        o << "]}";
    }
    o << "],\"permutation\":[";
    for (size_t i = 0; i < cs.permutation.size(); i++) o << (i ? "," : "") << "[\"" << kind_name(cs.permutation[i].kind) << "\"," << cs.permutation[i].index << "]";
    o << "]";
    const char* qn[3] = {"advice_queries", "fixed_queries", "instance_queries"};
    const std::vector<Query>* qv[3] = {&cs.advice_queries, &cs.fixed_queries, &cs.instance_queries};
    for (int t = 0; t < 3; t++) {
        o << ",\"" << qn[t] << "\":[";
        for (size_t i = 0; i < qv[t]->size(); i++) o << (i ? "," : "") << "[" << (*qv[t])[i].column << "," << (*qv[t])[i].rotation << "]";
        o << "]";
    }
    o << "}";
    c.describe = o.str();
}

static int circuit_create(int kind, unsigned k, unsigned bits, bzh_circuit** out) {
    std::unique_ptr<bzh_circuit> cp(new bzh_circuit());
    bzh_circuit& c = *cp;
    c.kind = kind;
    c.k = k;
    c.bits = bits;
    switch (kind) {
        case BZH_CIRCUIT_SHOT: c.shot = shot_configure(c.cs); c.num_instance_rows = 4; break;
        case BZH_CIRCUIT_BOARD: c.board = board_configure(c.cs); c.num_instance_rows = 2; break;
        case BZH_CIRCUIT_NUM2BITS_TEST: c.bitify = bitify_test_configure(c.cs, true); break;
        case BZH_CIRCUIT_BITS2NUM_TEST: c.bitify = bitify_test_configure(c.cs, false); break;
        default: return BZH_E_ARG;
    }
    if (((size_t)1 << k) < (size_t)c.cs.minimum_rows()) return BZH_E_RANGE;
    c.keygen.init(c.cs, k, true, false);
    Layouter lay(c.keygen, c.cs.constants);
    AnyInput in = default_input(kind);
    run_synthesize(c, lay, in);
    c.region_starts = lay.regions;
    for (auto& kv : lay.columns) {
        if (kv.first.kind == ADVICE) c.rows_used = std::max(c.rows_used, kv.second);
    }
    const std::vector<std::vector<Fp>> sel_polys = c.cs.compress_selectors(c.keygen.selectors);
    for (auto& p : sel_polys) c.keygen.fixed.push_back(p);
    build_blob_and_describe(c);
    *out = cp.release();
    return BZH_OK;
}

// rows [0, stride) of every (proof, column) come from the compact staged block, the rest of the n rows are zero
__global__ void __launch_bounds__(256) k_expand_advice(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n, size_t stride) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x, pc = blockIdx.y;   // i indexes 16-byte halves of the n elements
    if (i >= 2 * n) return;
    dst[pc * 2 * n + i] = (i < 2 * stride) ? src[pc * 2 * stride + i] : make_uint4(0, 0, 0, 0);
}

struct BatchInputs {
    const uint64_t* a = nullptr;  // shot: boards            | board: ship commitments (10 x 4) | bitify: value (canonical)
    const uint64_t* b = nullptr;  // shot: trapdoors         | board: boards                    | bitify: binary
    const uint64_t* c = nullptr;  // shot: shots             | board: trapdoors
    const uint64_t* d = nullptr;  // shot: hits
};
static void input_at(const bzh_circuit& c, const BatchInputs& bi, size_t i, AnyInput& in) {
    auto fq = [](const uint64_t* l) {
        Fq v;
        if (!Fq::from_limbs(l, &v)) throw GameError("trapdoor is not a canonical scalar");
        return v;
    };
    switch (c.kind) {
        case BZH_CIRCUIT_SHOT:
            in.shot.board = BinaryValue::from_limbs(bi.a + 4 * i);
            in.shot.trapdoor = fq(bi.b + 4 * i);
            in.shot.shot = BinaryValue::from_limbs(bi.c + 4 * i);
            in.shot.hit = BinaryValue::from_limbs(bi.d + 4 * i);
            break;
        case BZH_CIRCUIT_BOARD:
            for (int j = 0; j < 10; j++) in.board.ship_commitments[j] = BinaryValue::from_limbs(bi.a + 4 * (10 * i + j));
            in.board.board = BinaryValue::from_limbs(bi.b + 4 * i);
            in.board.trapdoor = fq(bi.c + 4 * i);
            break;
        default:
            if (!Fp::from_limbs(bi.a + 4 * i, &in.value)) throw GameError("value is not canonical");
            in.binary = BinaryValue::from_limbs(bi.b + 4 * i);
    }
}

// synthesise `batch` witnesses into compact blocks [proof][num_advice][stride] of Montgomery limbs
static int synthesize_compact(const bzh_circuit& c, size_t batch, const BatchInputs& bi, Fp* compact, size_t stride, uint64_t* instances,
                              unsigned threads, std::string* err) {
    const size_t na = (size_t)c.cs.num_advice;
    std::atomic<size_t> next{0};
    std::atomic<int> status{BZH_OK};
    std::mutex emu;
    auto worker = [&] {
        Assembly as;
        for (size_t i; (i = next.fetch_add(1)) < batch;) {
            if (status.load() != BZH_OK) return;
            try {
                Fp* out = compact + i * na * stride;
                std::fill(out, out + na * stride, Fp::zero());
                as.init(c.cs, c.k, false, true, out, stride);
                as.usable_rows = c.keygen.usable_rows;
                Layouter lay(as, c.cs.constants);
                lay.known_starts = &c.region_starts;
                AnyInput in;
                input_at(c, bi, i, in);
                const std::vector<Fp> inst = run_synthesize(c, lay, in);
                if (instances) {
                    for (size_t r = 0; r < inst.size(); r++) inst[r].to_limbs(instances + (i * inst.size() + r) * 4);
                }
            } catch (const std::exception& e) {
                std::lock_guard<std::mutex> g(emu);
                if (err) *err = e.what();
                status.store(BZH_E_RANGE);
                return;
            }
        }
    };
    if (!threads) threads = std::max(1u, std::min(16u, bzh::host_thread_budget()));
    threads = (unsigned)std::min<size_t>(threads, batch);
    if (threads <= 1) {
        worker();
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; t++) pool.emplace_back(worker);
        for (auto& t : pool) t.join();
    }
    return status.load();
}

// ---- BZH_SYNTH_DEVICE: what the kernels of csrc/synthesize_device.hip need from the circuit object ------------------------------
// The regions in the order the two `synthesize` functions of chips.hpp assign them; the rows come from region_starts.
static int synth_layout_of(const bzh_circuit& c, bzh::SynLayout* out) {
    using namespace bzh;
    SynLayout L;
    memset(&L, 0, sizeof(L));
    const bool shot = c.kind == BZH_CIRCUIT_SHOT;
    if (!shot && c.kind != BZH_CIRCUIT_BOARD) return BZH_E_ARG;
    const std::vector<size_t>& rs = c.region_starts;
    if (rs.size() != (shot ? 12u : 35u) || (size_t)c.cs.num_advice < 11) return BZH_E_ARG;
    L.kind = (uint32_t)c.kind;
    L.n = (uint32_t)c.keygen.n;
    L.rows_used = (uint32_t)c.rows_used;
    L.num_advice = (uint32_t)c.cs.num_advice;
    L.in_words = shot ? 16 : 48;
    for (int i = 0; i < 10; i++) L.col[i] = (uint32_t)(shot ? c.shot.advice[i] : c.board.advice[i]).index;
    L.col[10] = (uint32_t)(shot ? c.shot.input : c.board.advice[10]).index;
    L.src_board = shot ? 0 : 10;
    L.src_trapdoor = shot ? 1 : 11;
    static const int ship_len[5] = {5, 4, 3, 3, 2};
    for (int i = 0; i < 5; i++) {
        L.place_len[i] = (uint32_t)ship_len[i];
        for (int j = 0; j < BOARD_SIZE; j++) {
            if (!(j % 10 + ship_len[i] > 10)) L.place_mask[i][j / 64] |= (uint64_t)1 << (j % 64);
        }
    }
    uint32_t r = 0;
    auto add = [&](uint32_t type, uint32_t rows, uint32_t arg) { L.reg[r] = SynRegion{type, (uint32_t)rs[r], rows, arg}, r++; };
    const uint32_t B = BOARD_SIZE;
    if (shot) {
        L.load = (uint32_t)rs[0];
        add(SYN_R_SHOT_LOAD, 5, 0);
        add(SYN_R_BITIFY, B + 1, 0 | 5 << 8);      // board
        add(SYN_R_BITIFY, B + 1, 2 | 5 << 8);      // shot
        add(SYN_R_SHOT_SUM, B + 1, 0);
        add(SYN_R_SHOT_OUT, 1, 0);
    } else {
        L.load = (uint32_t)rs[0];
        add(SYN_R_BOARD_LOAD, 1, 0);
        for (uint32_t i = 0; i < 10; i++) add(SYN_R_BITIFY, B + 1, i | 0 << 8);
        for (uint32_t i = 0; i < 5; i++) {
            add(SYN_R_PLACE_A, B, i);
            add(SYN_R_PLACE_B, B + 1, i);
            add(SYN_R_PLACE_C, 1, i);
        }
        add(SYN_R_TRANSPOSE, B, 0);
        add(SYN_R_BITIFY, B + 1, 10 | 0 << 8);     // bits2num of the board bits
    }
    // pedersen_synthesize's seven regions
    L.inc[0] = (uint32_t)rs[r];
    add(SYN_R_BF_Z, ECC_NUM_WINDOWS + 1, 0);
    L.add[0] = (uint32_t)rs[r];
    add(SYN_R_SKIP, 2, 0);
    add(SYN_R_WITNESS, 14, 0);
    add(SYN_R_CANON, 3, 0);
    L.inc[1] = (uint32_t)rs[r];
    add(SYN_R_FW_WIN, ECC_NUM_WINDOWS, 0);
    L.add[1] = (uint32_t)rs[r];
    add(SYN_R_SKIP, 2, 0);
    L.final_add = (uint32_t)rs[r];
    add(SYN_R_SKIP, 2, 0);
    L.nregions = r;
    if (r != rs.size()) return BZH_E_ARG;
    for (uint32_t i = 0; i < r; i++) {
        if ((size_t)L.reg[i].start + L.reg[i].rows > c.rows_used || c.rows_used > c.keygen.n) return BZH_E_ARG;   // every write stays inside the tensor
    }
    for (int i = 0; i < 11; i++) {
        if (L.col[i] >= L.num_advice) return BZH_E_ARG;
    }
    *out = L;
    return BZH_OK;
}
// points[w][k] and u[w][k] of V then R as the kernels gather them: x, y, u in Montgomery form
static const std::vector<uint32_t>& synth_table() {
    static std::once_flag once;
    static std::vector<uint32_t> tbl;
    std::call_once(once, [] {
        const BoardFixedBases& fb = fixed_bases();
        tbl.resize(bzh::SYN_TBL_ENTRIES * bzh::SYN_TBL_WORDS);
        uint32_t* o = tbl.data();
        for (const FixedBase* b : {&fb.v, &fb.r}) {
            for (int w = 0; w < ECC_NUM_WINDOWS; w++) {
                for (int k = 0; k < ECC_H; k++, o += bzh::SYN_TBL_WORDS) {
                    memcpy(o, b->points[w][k].x.l, 32);
                    memcpy(o + 8, b->points[w][k].y.l, 32);
                    memcpy(o + 16, b->u[w][k].fe.l, 32);
                }
            }
        }
    });
    return tbl;
}

static thread_local std::string g_circuit_error;

}  // namespace

namespace bzh {
int synth_layout(const bzh_circuit* c, SynLayout* out) { return (c && out) ? synth_layout_of(*c, out) : BZH_E_ARG; }
const uint32_t* synth_table_host() { return synth_table().data(); }
}  // namespace bzh

extern "C" {

int bzh_circuit_create(int kind, unsigned k, unsigned bits, bzh_circuit** out) {
    if (!out || k < 4 || k > 24) return BZH_E_ARG;
    if ((kind == BZH_CIRCUIT_NUM2BITS_TEST || kind == BZH_CIRCUIT_BITS2NUM_TEST) && (bits < 1 || bits > 256)) return BZH_E_ARG;
    try {
        return circuit_create(kind, k, bits, out);
    } catch (const SynthesisError& e) {
        g_circuit_error = e.what();
        return BZH_E_RANGE;   // not enough rows for this k
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        return BZH_E_ARG;
    }
}
int bzh_circuit_free(bzh_circuit* c) {
    delete c;
    return BZH_OK;
}
const char* bzh_circuit_last_error(void) { return g_circuit_error.c_str(); }
int bzh_circuit_blob(const bzh_circuit* c, uint8_t* out, size_t cap, size_t* len) {
    if (!c || !len) return BZH_E_ARG;
    *len = c->blob.size();
    if (!out) return BZH_OK;
    if (cap < c->blob.size()) return BZH_E_RANGE;
    memcpy(out, c->blob.data(), c->blob.size());
    return BZH_OK;
}
int bzh_circuit_describe(const bzh_circuit* c, char* out, size_t cap, size_t* len) {
    if (!c || !len) return BZH_E_ARG;
    *len = c->describe.size() + 1;
    if (!out) return BZH_OK;
    if (cap < *len) return BZH_E_RANGE;
    memcpy(out, c->describe.c_str(), *len);
    return BZH_OK;
}
int bzh_circuit_info(const bzh_circuit* c, uint32_t* num_advice, uint32_t* num_instance_rows, uint32_t* n_rows, uint32_t* rows_used,
                     uint32_t* num_gates, uint32_t* num_regions) {
    if (!c) return BZH_E_ARG;
    if (num_advice) *num_advice = (uint32_t)c->cs.num_advice;
    if (num_instance_rows) *num_instance_rows = (uint32_t)c->num_instance_rows;
    if (n_rows) *n_rows = (uint32_t)c->keygen.n;
    if (rows_used) *rows_used = (uint32_t)c->rows_used;
    if (num_gates) *num_gates = (uint32_t)c->cs.gates.size();
    if (num_regions) *num_regions = (uint32_t)c->keygen.regions.size();
    return BZH_OK;
}

/* the verifying-key digest: halo2_proofs 0.2.0 plonk.rs VerifyingKey::hash_into (UPSTREAM) -- Blake2b-512, personal
 * "Halo2-Verify-Key", over (len as u64 LE) || format!("{:?}", vk.pinned()), reduced with from_bytes_wide */
int bzh_vk_digest(const char* pinned_debug, size_t len, uint8_t* out_repr) {
    if ((!pinned_debug && len) || !out_repr) return BZH_E_ARG;
    bzh::Blake2b h;
    h.init(64, (const uint8_t*)"Halo2-Verify-Key");
    const uint64_t l64 = (uint64_t)len;
    uint8_t lb[8];
    for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(l64 >> (8 * i));
    h.update(lb, 8);
    h.update((const uint8_t*)pinned_debug, len);
    uint8_t d[64];
    h.finalize(d);
    const Fp v = bzh::h_from_u512<bzh::FpParams>(d);   // from_bytes_wide: the 512-bit little-endian integer mod p
    v.to_repr(out_repr);
    return BZH_OK;
}
int bzh_circuit_set_vk_repr(bzh_circuit* c, const uint8_t* repr) {
    if (!c || !repr) return BZH_E_ARG;
    Fp v;
    if (!Fp::from_repr(repr, &v)) return BZH_E_RANGE;   // Fp::from_repr(..) is None upstream
    if (c->blob.size() < BZH_CIRCUIT_BLOB_VK_REPR_OFFSET + 32) return BZH_E_ARG;
    memcpy(c->blob.data() + BZH_CIRCUIT_BLOB_VK_REPR_OFFSET, repr, 32);
    c->vk_placeholder = false;
    return BZH_OK;
}
int bzh_circuit_vk_repr(const bzh_circuit* c, uint8_t* out_repr, int* is_placeholder) {
    if (!c || c->blob.size() < BZH_CIRCUIT_BLOB_VK_REPR_OFFSET + 32) return BZH_E_ARG;
    if (out_repr) memcpy(out_repr, c->blob.data() + BZH_CIRCUIT_BLOB_VK_REPR_OFFSET, 32);
    if (is_placeholder) *is_placeholder = c->vk_placeholder ? 1 : 0;
    return BZH_OK;
}

// BZH_SYNTH_DEVICE: the inputs are checked and staged here, the witness is computed by csrc/synthesize_device.hip's kernels
// step one, "check and pack the inputs": no device use (bzh::synth_pack_inputs hands it to the prover's translation unit)
static int synthesize_device_pack(const bzh_circuit* c, size_t batch, const BatchInputs& bi, bzh::SynLayout* layout, std::vector<uint64_t>* packed,
                                  std::string* err) {
    bzh::SynLayout& L = *layout;
    BZH_TRY(bzh::synth_layout(c, &L));
    const bool shot = c->kind == BZH_CIRCUIT_SHOT;
    packed->assign(batch * L.in_words, 0);
    std::vector<uint64_t>& in = *packed;
    try {
        // the host path's refusals that depend on the inputs alone, before anything is launched, with its error texts
        for (size_t i = 0; i < batch; i++) {
            AnyInput a;
            input_at(*c, bi, i, a);
            uint64_t* o = in.data() + i * L.in_words;
            if (shot) {
                memcpy(o, bi.a + 4 * i, 32), memcpy(o + 4, bi.b + 4 * i, 32), memcpy(o + 8, bi.c + 4 * i, 32), memcpy(o + 12, bi.d + 4 * i, 32);
            } else {
                for (int j = 0; j < 5; j++) (void)a.board.ship_commitments[2 * j].zip(a.board.ship_commitments[2 * j + 1]);
                memcpy(o, bi.a + 40 * i, 320), memcpy(o + 40, bi.b + 4 * i, 32), memcpy(o + 44, bi.c + 4 * i, 32);
            }
        }
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        if (err) *err = e.what();
        return BZH_E_RANGE;
    }
    return BZH_OK;
}
// step two, the run: enqueue, then read back
static int synthesize_device(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const BatchInputs& bi, uint64_t* advice, uint64_t* instances) {
    bzh::SynLayout L;
    std::vector<uint64_t> in;
    std::string err;
    const int prc = synthesize_device_pack(c, batch, bi, &L, &in, &err);
    if (prc) {
        if (prc == BZH_E_RANGE) ctx->last_error = err;
        return prc;
    }
    const bool shot = c->kind == BZH_CIRCUIT_SHOT;
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> status(batch);
    std::vector<uint64_t> cm(instances ? batch * 8 : 0);
    bzh::SynRun run;
    run.layout = &L, run.batch = batch, run.inputs = in.data(), run.table = bzh::synth_table_host(), run.d_advice = (uint32_t*)advice;
    run.commitments = instances ? cm.data() : nullptr, run.status = status.data();
    BZH_TRY(bzh::synth_device_run(ctx, run));
    for (size_t i = 0; i < batch; i++) {
        if (!status[i]) continue;
        const char* what = bzh::syn_status_text(status[i]);
        g_circuit_error = what;
        ctx->last_error = what;
        return BZH_E_RANGE;
    }
    if (instances) {
        const size_t ni = (size_t)c->num_instance_rows;
        for (size_t i = 0; i < batch; i++) {
            uint64_t* o = instances + i * ni * 4;
            memcpy(o, cm.data() + i * 8, 64);
            if (shot) {
                const uint64_t pub[2][4] = {{bi.c[4 * i], bi.c[4 * i + 1], 0, 0}, {bi.d[4 * i], bi.d[4 * i + 1], 0, 0}};   // from_u128(lower_u128())
                memcpy(o + 8, pub, 64);
            }
        }
    }
    return BZH_OK;
}

}  // extern "C"
namespace bzh {
int synth_shape(const bzh_circuit* c, SynShape* out) {
    if (!c || !out) return BZH_E_ARG;
    out->kind = c->kind, out->n = c->keygen.n, out->num_advice = (size_t)c->cs.num_advice, out->num_instance = (size_t)c->cs.num_instance,
    out->inst_rows = (size_t)c->num_instance_rows;
    return BZH_OK;
}
int synth_pack_inputs(const bzh_circuit* c, size_t batch, const uint64_t* a, const uint64_t* b, const uint64_t* c_in, const uint64_t* d,
                      SynLayout* layout, std::vector<uint64_t>* in, std::string* err) {
    if (!c || !batch || !layout || !in || !a || !b || !c_in || (c->kind == BZH_CIRCUIT_SHOT && !d)) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = a, bi.b = b, bi.c = c_in, bi.d = d;
    return synthesize_device_pack(c, batch, bi, layout, in, err);
}
}  // namespace bzh
extern "C" {

static int synthesize_any(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const BatchInputs& bi, uint64_t* advice, int form, int mem,
                          uint64_t* instances, unsigned threads, int where = BZH_SYNTH_HOST) {
    if (!c || !batch || batch > 65536 || !advice) return BZH_E_ARG;
    if ((form != BZH_FORM_CANONICAL && form != BZH_FORM_MONTGOMERY) || (mem != BZH_MEM_HOST && mem != BZH_MEM_DEVICE)) return BZH_E_ARG;
    if (mem == BZH_MEM_DEVICE && (!ctx || form != BZH_FORM_MONTGOMERY)) return BZH_E_ARG;
    if (where != BZH_SYNTH_HOST && where != BZH_SYNTH_DEVICE) return BZH_E_ARG;
    if (where == BZH_SYNTH_DEVICE) {
        if (!ctx || mem != BZH_MEM_DEVICE || form != BZH_FORM_MONTGOMERY) return BZH_E_ARG;
        return synthesize_device(ctx, c, batch, bi, advice, instances);
    }
    const size_t na = (size_t)c->cs.num_advice, n = c->keygen.n, stride = std::max<size_t>(c->rows_used, 1);
    std::string err;
    if (mem == BZH_MEM_HOST) {
        std::vector<Fp> compact(batch * na * stride);
        const int rc = synthesize_compact(*c, batch, bi, compact.data(), stride, instances, threads, &err);
        if (rc) {
            g_circuit_error = err;
            if (ctx) ctx->last_error = err;
            return rc;
        }
        memset(advice, 0, batch * na * n * 32);
        for (size_t pc = 0; pc < batch * na; pc++) {
            for (size_t r = 0; r < stride; r++) {
                uint64_t* dst = advice + (pc * n + r) * 4;
                if (form == BZH_FORM_MONTGOMERY) {
                    memcpy(dst, compact[pc * stride + r].fe.l, 32);
                } else {
                    compact[pc * stride + r].to_limbs(dst);
                }
            }
        }
        return BZH_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BZH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    char* slot = nullptr;
    const size_t bytes = batch * na * stride * 32;
    int rc = bzh::h2d_stage(ctx, bytes, &slot);
    if (rc) return rc;
    rc = synthesize_compact(*c, batch, bi, (Fp*)slot, stride, instances, threads, &err);   // pinned staging: circuit/hostfield.hpp asserts Fp's size and alignment
    if (rc) {
        g_circuit_error = err;
        ctx->last_error = err;
        return rc;
    }
    dim3 grid((unsigned)((2 * n + 255) / 256), (unsigned)(batch * na));
    hipLaunchKernelGGL(k_expand_advice, grid, dim3(256), 0, ctx->stream, (uint4*)advice, (const uint4*)slot, n, stride);
    BZH_HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

int bzh_synthesize_shot(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* boards, const uint64_t* trapdoors, const uint64_t* shots,
                        const uint64_t* hits, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads) {
    if (!c || c->kind != BZH_CIRCUIT_SHOT || !boards || !trapdoors || !shots || !hits) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = boards, bi.b = trapdoors, bi.c = shots, bi.d = hits;
    return synthesize_any(ctx, c, batch, bi, advice, form, mem, instances, threads);
}
int bzh_synthesize_board(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* ship_commitments, const uint64_t* boards,
                         const uint64_t* trapdoors, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads) {
    if (!c || c->kind != BZH_CIRCUIT_BOARD || !ship_commitments || !boards || !trapdoors) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = ship_commitments, bi.b = boards, bi.c = trapdoors;
    return synthesize_any(ctx, c, batch, bi, advice, form, mem, instances, threads);
}
int bzh_synthesize_shot_with(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* boards, const uint64_t* trapdoors, const uint64_t* shots,
                             const uint64_t* hits, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads, int where) {
    if (!c || c->kind != BZH_CIRCUIT_SHOT || !boards || !trapdoors || !shots || !hits) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = boards, bi.b = trapdoors, bi.c = shots, bi.d = hits;
    return synthesize_any(ctx, c, batch, bi, advice, form, mem, instances, threads, where);
}
int bzh_synthesize_board_with(bzh_ctx* ctx, const bzh_circuit* c, size_t batch, const uint64_t* ship_commitments, const uint64_t* boards,
                              const uint64_t* trapdoors, uint64_t* advice, int form, int mem, uint64_t* instances, unsigned threads, int where) {
    if (!c || c->kind != BZH_CIRCUIT_BOARD || !ship_commitments || !boards || !trapdoors) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = ship_commitments, bi.b = boards, bi.c = trapdoors;
    return synthesize_any(ctx, c, batch, bi, advice, form, mem, instances, threads, where);
}
int bzh_synthesize_bitify_test(const bzh_circuit* c, const uint64_t* value, const uint64_t* binary, uint64_t* advice) {
    if (!c || (c->kind != BZH_CIRCUIT_NUM2BITS_TEST && c->kind != BZH_CIRCUIT_BITS2NUM_TEST) || !value || !binary) return BZH_E_ARG;
    BatchInputs bi;
    bi.a = value, bi.b = binary;
    return synthesize_any(nullptr, c, 1, bi, advice, BZH_FORM_CANONICAL, BZH_MEM_HOST, nullptr, 1);
}

/* game / witness marshalling (src/utils/{ship,deck,board,shot}.rs) */
int bzh_board_witness(const int8_t* ships, const int32_t* options, uint64_t* ship_commitments, uint64_t* state) {
    if (!ships || !ship_commitments || !state) return BZH_E_ARG;
    try {
        Board b;
        int opts[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 5; i++) {
            const int8_t *s = ships + 3 * i;
            if (s[0] >= 0) b.deck.add(i, s[0], s[1], s[2] != 0);
            if (options) opts[i] = options[i];
        }
        BinaryValue w[10];
        b.witness(opts, w);
        for (int i = 0; i < 10; i++) memcpy(ship_commitments + 4 * i, w[i].w, 32);
        const BinaryValue st = b.state(opts);
        memcpy(state, st.w, 32);
        return BZH_OK;
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        return BZH_E_RANGE;
    }
}
int bzh_shot_serialize(const uint8_t* xs, const uint8_t* ys, size_t count, uint64_t* out) {
    if (!xs || !ys || !out) return BZH_E_ARG;
    try {
        const BinaryValue b = serialize_shot(xs, ys, (int)count);
        memcpy(out, b.w, 32);
        return BZH_OK;
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        return BZH_E_RANGE;
    }
}
/* native Pedersen commitment on the host from the circuit's own window tables (src/utils/pedersen.rs:17-28) */
int bzh_pedersen_commit_host(const uint64_t* message, const uint64_t* trapdoor, uint64_t* out_xy) {
    if (!message || !trapdoor || !out_xy) return BZH_E_ARG;
    try {
        Fp m;
        Fq t;
        if (!Fp::from_limbs(message, &m) || !Fq::from_limbs(trapdoor, &t)) return BZH_E_RANGE;
        const Aff a = pedersen_commit_native(fixed_bases(), m, t);
        Fp(a.x).to_limbs(out_xy);
        Fp(a.y).to_limbs(out_xy + 4);
        return BZH_OK;
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        return BZH_E_RANGE;
    }
}
/* fixed-base tables of the in-circuit Pedersen commitment: base 0 = V, 1 = R; z: 85 u64, u: 85 x 8 x 4 canonical limbs,
 * lagrange: 85 x 8 x 4 canonical limbs (src/utils/constants/fixed_bases/board_commit_{v,r}.rs:17-2927) */
int bzh_fixed_base_tables(int base, uint64_t* z, uint64_t* u, uint64_t* lagrange) {
    if (base < 0 || base > 1) return BZH_E_ARG;
    try {
        const FixedBase& fb = base == 0 ? fixed_bases().v : fixed_bases().r;
        for (int w = 0; w < ECC_NUM_WINDOWS; w++) {
            if (z) z[w] = fb.z[w];
            for (int k = 0; k < ECC_H; k++) {
                if (u) fb.u[w][k].to_limbs(u + ((size_t)w * ECC_H + k) * 4);
                if (lagrange) fb.lagrange[w][k].to_limbs(lagrange + ((size_t)w * ECC_H + k) * 4);
            }
        }
        return BZH_OK;
    } catch (const std::exception& e) {
        g_circuit_error = e.what();
        return BZH_E_HIP;
    }
}

}  // extern "C"
