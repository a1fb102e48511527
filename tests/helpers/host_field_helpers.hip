// Test program (not product code): the host helpers of csrc/host_field.hpp -- square root, point decompression, roots of
// unity, the Jacobi symbol, batch inversion, interpolation, Jacobian / XYZZ -> affine -- driven by a command file, one command per line, one answer line each.
// tests/test_host_field_cpu.py writes the commands and compares the answers with oracle/pasta.py.  All values are 64 hex
// digits, big-endian, canonical unless a form says otherwise.
//   sqrt F a                         -> "ok r" | "none"
//   decompress C bytes32             -> "ok x y" | "reject"          (bytes32: the 32 encoded bytes as they lie in memory)
//   omega F log_n                    -> "w"
//   binv F skip_zeros n v_0 .. v_n-1 -> "ok 1/v_0 .." | "fail"
//   interp F np x_0 .. x_np-1 y_0 .. y_np-1 -> "ok c_0 .. c_np-1" (coefficients, lowest first) | "fail" (two points coincide)
//   jac C in_form out_form n X Y Z.. -> "x y .."                      (limbs in the given forms, 0 canonical, 1 Montgomery)
//   jacobi F a                       -> "1" | "-1" | "0"
//   xyzz C n X Y ZZ ZZZ ..           -> "x y .."                      (h_xyzz_to_affine)
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "host_field.hpp"
using namespace bzh;

static void parse(const std::string& h, uint64_t l[4]) {
    for (int i = 0; i < 4; i++) l[3 - i] = std::stoull(h.substr(16 * i, 16), nullptr, 16);
}
static std::string hex(const uint64_t l[4]) {
    char buf[65];
    snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)l[3], (unsigned long long)l[2], (unsigned long long)l[1],
             (unsigned long long)l[0]);
    return buf;
}
template <class P>
static Fe<P> read_fe(std::istream& in, int form = BZH_FORM_CANONICAL) {
    std::string h;
    in >> h;
    uint64_t l[4];
    parse(h, l);
    return fe_from_u64<P>(l, form);
}
template <class P>
static std::string show(const Fe<P>& v, int form = BZH_FORM_CANONICAL) {
    uint64_t l[4];
    fe_to_u64<P>(l, v, form);
    return hex(l);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        int id = -1;
        in >> cmd >> id;
        std::string out;
        int rc = BZH_E_ARG;
        if (cmd == "sqrt") {
            rc = with_field(id, [&](auto p) {
                using P = decltype(p);
                Fe<P> r;
                out = h_sqrt(read_fe<P>(in), r) ? "ok " + show(r) : "none";
                return BZH_OK;
            });
        } else if (cmd == "decompress") {
            rc = with_curve(id, [&](auto c) {
                std::string h;
                in >> h;
                uint8_t raw[32];
                for (int i = 0; i < 32; i++) raw[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
                uint64_t xy[8];
                out = h_decompress<decltype(c)>(raw, xy) ? "ok " + hex(xy) + " " + hex(xy + 4) : "reject";
                return BZH_OK;
            });
        } else if (cmd == "omega") {
            rc = with_field(id, [&](auto p) {
                unsigned log_n = 0;
                in >> log_n;
                out = show(h_omega<decltype(p)>(log_n));
                return BZH_OK;
            });
        } else if (cmd == "binv") {
            rc = with_field(id, [&](auto p) {
                using P = decltype(p);
                int skip = 0;
                size_t n = 0;
                in >> skip >> n;
                std::vector<Fe<P>> v(n);
                for (auto& e : v) e = read_fe<P>(in);
                const std::vector<Fe<P>> before = v;
                if (h_batch_invert(v.data(), n, skip != 0)) {
                    out = "ok";
                    for (auto& e : v) out += " " + show(e);
                } else {
                    out = "fail";
                    for (size_t i = 0; i < n; i++)
                        if (!fe_eq(v[i], before[i])) out = "fail-but-wrote";
                }
                return BZH_OK;
            });
        } else if (cmd == "interp") {
            rc = with_field(id, [&](auto p) {
                using P = decltype(p);
                size_t np = 0;
                in >> np;
                std::vector<Fe<P>> x(np), y(np), den(np, fe_one<P>()), c(np + 1, fe_one<P>());   // c[np]: a guard past the output
                for (auto& e : x) e = read_fe<P>(in);
                for (auto& e : y) e = read_fe<P>(in);
                for (size_t j = 0; j < np; j++)
                    for (size_t m = 0; m < np; m++)
                        if (m != j) den[j] = fe_mul(den[j], fe_sub(x[j], x[m]));
                if (!h_batch_invert(den.data(), np)) {
                    out = "fail";
                    return BZH_OK;
                }
                h_interpolate(x.data(), y.data(), den.data(), np, c.data());
                out = fe_eq(c[np], fe_one<P>()) ? "ok" : "wrote-past-the-end";
                for (size_t i = 0; i < np; i++) out += " " + show(c[i]);
                return BZH_OK;
            });
        } else if (cmd == "jac") {
            rc = with_curve(id, [&](auto c) {
                int in_form = 0, out_form = 0;
                size_t n = 0;
                in >> in_form >> out_form >> n;
                std::vector<uint64_t> xyz(12 * n + 1), xy(8 * n + 1, ~(uint64_t)0);
                for (size_t i = 0; i < 3 * n; i++) {
                    std::string h;
                    in >> h;
                    parse(h, &xyz[4 * i]);
                }
                h_jac_to_affine<typename decltype(c)::Base>(xyz.data(), n, in_form, out_form, xy.data());
                for (size_t i = 0; i < 2 * n; i++) out += (i ? " " : "") + hex(&xy[4 * i]);
                return BZH_OK;
            });
        } else if (cmd == "jacobi") {
            rc = with_field(id, [&](auto p) {
                using P = decltype(p);
                out = std::to_string(h_jacobi(fe_from_mont(read_fe<P>(in))));
                return BZH_OK;
            });
        } else if (cmd == "xyzz") {
            rc = with_curve(id, [&](auto c) {
                using P = typename decltype(c)::Base;
                size_t n = 0;
                in >> n;
                std::vector<Xyzz<P>> v(n);
                for (auto& e : v) e.x = read_fe<P>(in), e.y = read_fe<P>(in), e.zz = read_fe<P>(in), e.zzz = read_fe<P>(in);
                std::vector<Affine<P>> a(n + 1);
                a[n].x = a[n].y = fe_one<P>();   // a guard past the output
                h_xyzz_to_affine(v.data(), n, a.data());
                if (!fe_eq(a[n].x, fe_one<P>()) || !fe_eq(a[n].y, fe_one<P>())) out = "wrote-past-the-end ";
                for (size_t i = 0; i < n; i++) out += (i ? " " : "") + show(a[i].x) + " " + show(a[i].y);
                return BZH_OK;
            });
        }
        if (rc) out = "bad command";
        std::cout << out << "\n";
    }
    return 0;
}
