// tests/host/test_circuit_words.cpp -- sipp::CircuitData::set_input_map / prove_words (include/sipp_host.hpp over
// sipp_circuit_set_input_map / sipp_circuit_prove_words) for a caller with host memory only and no array library: a circuit as DATA
// (fixture written by tests/test_gpu_circuit_words_cpp.py), the map, the words; the proof goes to <out> for the test to compare.
//
//   test_circuit_words <fixture.bin> <out.bin>      GPU
//
// fixture, u64 words: header[16] = degree_bits, num_wires, num_routed, num_constants, num_selectors, num_gates, program_words, n_gens,
//   n_levels, n_rows, n_copies, n_public_inputs, max_degree, n_map, n_words, n_extra | fri params (7 + 32) | gates (6 each) | programs
//   | generators (8 each) | rows | level_offsets | copy_src | copy_dst | copy_offsets | constants_sigmas | map cells | map sources
//   | words | extra | public inputs
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>

#include "sipp_host.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int refused(const std::function<void()>& call) {
    try {
        call();
    } catch (const sipp::Error& e) {
        return e.status();
    }
    return SIPP_OK;
}

static int run(const char* path, const char* out_path) {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    CHECK(in);
    std::vector<uint64_t> w((size_t)in.tellg() / 8);
    in.seekg(0);
    in.read(reinterpret_cast<char*>(w.data()), (std::streamsize)(w.size() * 8));
    size_t pos = 0;
    auto next = [&](size_t count) {
        if (pos + count > w.size()) {
            fprintf(stderr, "fixture too short\n");
            exit(2);
        }
        pos += count;
        return std::vector<uint64_t>(w.begin() + (std::ptrdiff_t)(pos - count), w.begin() + (std::ptrdiff_t)pos);
    };
    auto u32s = [&](size_t count) {
        const std::vector<uint64_t> q = next(count);
        return std::vector<uint32_t>(q.begin(), q.end());
    };
    const std::vector<uint64_t> h = next(16);
    const uint32_t degree_bits = (uint32_t)h[0], n_levels = (uint32_t)h[8];
    const size_t n = (size_t)1 << degree_bits, n_rows = h[9], n_copies = h[10], n_map = h[13], n_words = h[14], n_extra = h[15];
    const sipp_plonk_params params{(uint32_t)h[2], (uint32_t)h[12], 2};
    sipp_fri_params fri{};
    const std::vector<uint64_t> f = next(7 + SIPP_FRI_MAX_ROUNDS);
    fri.rate_bits = (uint32_t)f[0]; fri.cap_height = (uint32_t)f[1]; fri.pow_bits = (uint32_t)f[2]; fri.num_queries = (uint32_t)f[3];
    fri.pow_rule = (uint32_t)f[4]; fri.hiding = (uint32_t)f[5]; fri.n_rounds = (uint32_t)f[6];
    for (uint32_t i = 0; i < SIPP_FRI_MAX_ROUNDS; i++) fri.arity_bits[i] = (uint32_t)f[7 + i];
    std::vector<sipp_plonk_gate> gates(h[5]);
    for (auto& g : gates) {
        const std::vector<uint64_t> q = next(6);
        g = sipp_plonk_gate{(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3], (uint32_t)q[4], (uint32_t)q[5]};
    }
    const std::vector<uint64_t> pr = next(h[6]);
    const std::vector<int64_t> programs(pr.begin(), pr.end());
    std::vector<sipp_plonk_generator> gens(h[7]);
    for (auto& g : gens) {
        const std::vector<uint64_t> q = next(8);
        g = sipp_plonk_generator{(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], {(uint32_t)q[3], (uint32_t)q[4], (uint32_t)q[5], (uint32_t)q[6], (uint32_t)q[7]}};
    }
    const std::vector<uint32_t> rows = u32s(n_rows), level_offsets = u32s(n_levels + 1);
    const std::vector<uint64_t> copy_src = next(n_copies), copy_dst = next(n_copies);
    const std::vector<uint32_t> copy_offsets = u32s(n_levels + 1);
    const sipp_plonk_schedule_host sched{n_levels, rows.data(), level_offsets.data(), copy_src.data(), copy_dst.data(), copy_offsets.data()};
    const std::vector<uint64_t> constants_sigmas = next((size_t)(h[3] + h[2]) * n);
    const std::vector<uint64_t> cells = next(n_map), sources = next(n_map), words = next(n_words), extra = next(n_extra), statement = next(h[11]);
    CHECK(pos == w.size());
    const sipp_plonk_circuit circuit{(uint32_t)h[1], (uint32_t)h[3], (uint32_t)h[4], (uint32_t)gates.size(), gates.data(), programs.data(),
                                     (uint32_t)programs.size()};

    sipp::CircuitData data(0, degree_bits, params, fri, circuit, constants_sigmas, gens, &sched);
    CHECK(refused([&] { (void)data.prove_words(words, extra, statement); }) == SIPP_E_BADARG);           // no map yet
    data.set_input_map(cells, sources, n_words, n_extra);
    const sipp::ProofWithPublicInputs proof = data.prove_words(words, extra, statement);
    data.verify(proof);
    CHECK(proof.public_inputs == statement);
    // refusals leave the map in force: a source behind the staged words, a cell behind the table, lists of two lengths, fewer words
    std::vector<uint64_t> bad = sources;
    bad.back() = n_words + n_extra;
    CHECK(refused([&] { data.set_input_map(cells, bad, n_words, n_extra); }) == SIPP_E_BADARG);
    bad = cells;
    bad.front() = (uint64_t)circuit.num_wires * n;
    CHECK(refused([&] { data.set_input_map(bad, sources, n_words, n_extra); }) == SIPP_E_BADARG);
    bad.pop_back();
    CHECK(refused([&] { data.set_input_map(bad, sources, n_words, n_extra); }) == SIPP_E_BADARG);
    CHECK(refused([&] { (void)data.prove_words(std::vector<uint64_t>(words.begin(), words.end() - 1), extra, statement); }) == SIPP_E_BADARG);
    CHECK(data.prove_words(words, extra, statement).flat == proof.flat);
    // the same map again replaces the first
    data.set_input_map(cells, sources, n_words, n_extra);
    CHECK(data.prove_words(words, extra, statement).flat == proof.flat);
    std::ofstream o(out_path, std::ios::binary);
    o.write(reinterpret_cast<const char*>(proof.flat.data()), (std::streamsize)(proof.flat.size() * 8));
    o.write(reinterpret_cast<const char*>(data.circuit_digest), 32);
    printf("prove_words ok: %zu words from %zu pairs over %zu + %zu staged words\n", proof.flat.size(), n_map, n_words, n_extra);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <fixture.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    try {
        return run(argv[1], argv[2]);
    } catch (const sipp::Error& e) {
        fprintf(stderr, "sipp::Error %d: %s\n", e.status(), e.what());
        return 1;
    }
}
