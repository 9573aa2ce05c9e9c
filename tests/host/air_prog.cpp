// tests/host/air_prog.cpp -- air_read_gadgets (sipp_amd/csrc/air_prog.hpp: the one reading of an AIR program's gadget part that
// trace.hip and prover.hip build their tables from) against a second walk written here from the program format, for every AIR of
// data/air_tables.h.  CPU only; tests/test_host_air_prog.py builds and runs it, plain and under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "air_prog.hpp"
#include "air_tables.h"

static int fails = 0;
#define CHECK(cond, ...)                \
    do {                                \
        if (!(cond)) {                  \
            std::printf("FAIL air %d: ", air); \
            std::printf(__VA_ARGS__);   \
            std::printf("\n");          \
            fails++;                    \
        }                               \
    } while (0)

// the second reading: indices instead of a moving pointer, every read bounds-checked against prog_len
struct Walk {
    const int64_t* p;
    int64_t len, i = 0;
    bool ok = true;
    int64_t at(int64_t k) {
        if (k < 0 || k >= len) {
            ok = false;
            return 0;
        }
        return p[k];
    }
    void vec() { i += 2 + 5 * at(i + 1); }   // word, term count, five words per term
};

int main() {
    const int n_airs = (int)(sizeof(AIR_AIRS) / sizeof(AIR_AIRS[0]));
    long gadgets = 0, products = 0, polys = 0;
    for (int air = 0; air < n_airs; air++) {
        const air_spec_t& a = AIR_AIRS[air];
        const AirGadgets got = air_read_gadgets(a.prog, a.prog_len);

        // ---- the plain walk ----
        Walk w{a.prog, a.prog_len};
        std::vector<int64_t> off, group, np;
        std::vector<std::vector<int64_t>> prod;
        while (w.ok && w.i < w.len && w.at(w.i) == 1) {
            off.push_back(w.i);
            group.push_back(w.at(w.i + 6));
            w.i += 7;
            w.vec();
            const int64_t n_prod = w.at(w.i);
            w.i += 1;
            np.push_back(n_prod);
            prod.emplace_back();
            for (int64_t k = 0; k < n_prod && w.ok; k++) {
                prod.back().push_back(w.i);
                w.i += 1;
                w.vec();
                w.vec();
            }
            prod.back().push_back(w.i);
            const int64_t n_lin = w.at(w.i);
            w.i += 1;
            for (int64_t k = 0; k < n_lin && w.ok; k++) {
                w.i += 1;
                w.vec();
            }
        }
        CHECK(w.ok, "the plain walk left the program in its gadget part");
        const int64_t poly_start = w.i;

        // ---- the header's reading against it ----
        CHECK((int)got.gadgets.size() == a.n_gadgets, "gadget count %zu, n_gadgets %d", got.gadgets.size(), a.n_gadgets);
        CHECK(got.gadgets.size() == off.size(), "gadget count %zu, plain walk %zu", got.gadgets.size(), off.size());
        CHECK((int64_t)got.poly_off == poly_start, "POLY ops begin at %u, plain walk %lld", got.poly_off, (long long)poly_start);
        for (size_t g = 0; g < got.gadgets.size() && g < off.size(); g++) {
            const AirGadget& x = got.gadgets[g];
            const int64_t end = g + 1 < got.gadgets.size() ? (int64_t)got.gadgets[g + 1].off : (int64_t)got.poly_off;
            CHECK((int64_t)x.off == off[g] && x.group == group[g] && x.np == np[g], "gadget %zu: offset / group / products (%u, %lld, %lld) against (%lld, %lld, %lld)",
                  g, x.off, (long long)x.group, (long long)x.np, (long long)off[g], (long long)group[g], (long long)np[g]);
            CHECK(x.off < (uint32_t)a.prog_len && a.prog[x.off] == 1, "gadget %zu: offset %u does not point at an op word 1", g, x.off);
            CHECK(g == 0 || x.off > got.gadgets[g - 1].off, "gadget %zu: offsets not strictly increasing", g);
            CHECK(x.group == a.prog[x.off + 6], "gadget %zu: limb group is not w[6]", g);
            CHECK((int64_t)x.prod_off.size() == x.np + 1, "gadget %zu: %zu product offsets for %lld products", g, x.prod_off.size(), (long long)x.np);
            CHECK(x.prod_off.size() == prod[g].size(), "gadget %zu: product offset count against the plain walk", g);
            for (size_t k = 0; k < x.prod_off.size(); k++) {
                CHECK((int64_t)x.prod_off[k] > (int64_t)x.off && (int64_t)x.prod_off[k] < end, "gadget %zu: product offset %zu = %u outside (%u, %lld)", g, k,
                      x.prod_off[k], x.off, (long long)end);
                CHECK(k >= prod[g].size() || (int64_t)x.prod_off[k] == prod[g][k], "gadget %zu: product offset %zu against the plain walk", g, k);
                CHECK(k == 0 || x.prod_off[k] > x.prod_off[k - 1], "gadget %zu: product offsets not increasing at %zu", g, k);
            }
            gadgets++;
            products += (long)x.np;
        }
        // ---- the POLY ops from the reported start: word, monomial count, per monomial (word, k, k pairs); ends at prog_len exactly ----
        Walk q{a.prog, a.prog_len};
        q.i = got.poly_off;
        while (q.ok && q.i < q.len) {
            CHECK(q.at(q.i) == 2, "op word %lld at %lld in the POLY part", (long long)q.at(q.i), (long long)q.i);
            const int64_t nmono = q.at(q.i + 1);
            q.i += 2;
            for (int64_t m = 0; m < nmono && q.ok; m++) q.i += 2 + 2 * q.at(q.i + 1);
            polys++;
        }
        CHECK(q.ok && q.i == q.len, "the POLY walk ends at %lld, prog_len %lld", (long long)q.i, (long long)q.len);
    }
    std::printf("%d airs, %ld gadgets, %ld products, %ld POLY ops, %d failures\n", n_airs, gadgets, products, polys, fails);
    if (fails == 0) std::printf("air_prog ok\n");
    return fails ? 1 : 0;
}
