// sipp_amd/csrc/flow.hip -- from the points A, B of a SIPP instance to its three STARK proofs (host code only).
//
//   sipp_flow_prove    sipp_prove_native_ex (native.hip), then sipp_instance_prove (stark.hip) on the lists it produced
//   sipp_flows_prove   sipp_instances_prove with a producer in front: one host thread runs the native chain of instance 0, 1, ... on a
//                      ctx of its own while the slot workers prove the instances whose lists exist -- the latency-bound native stage
//                      of instance k + 1 beside the hash-bound proofs of instance k
// Everything here goes through the public C ABI (include/sipp_hip.h): no kernel, no access to the ctx.
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/sipp_hip.h"

namespace {

// the obligation lists of one instance, sized for n (a power of two): (n - 1) x 56, (n - 1) x 104, 2 log2 n x 296 u32
struct Lists {
    std::vector<uint32_t> rec[3];
    size_t num[3] = {0, 0, 0};
    void size_for(size_t n) {
        size_t lg = 0;
        while (((size_t)1 << lg) < n) lg++;
        num[SIPP_G1_EXP] = num[SIPP_G2_EXP] = n - 1;
        num[SIPP_FQ12_EXP] = 2 * lg;
        rec[SIPP_G1_EXP].assign(num[SIPP_G1_EXP] * SIPP_G1_IO_WORDS + 1, 0);  // + 1: data() of a kind without records is still a buffer
        rec[SIPP_G2_EXP].assign(num[SIPP_G2_EXP] * SIPP_G2_IO_WORDS + 1, 0);
        rec[SIPP_FQ12_EXP].assign(num[SIPP_FQ12_EXP] * SIPP_FQ12_IO_WORDS + 1, 0);
    }
};

// the native stage of one instance: sipp_prove_native_ex into `l`; a size that is no power of two gets that call's refusal
int native_stage(sipp_ctx* ctx, const uint32_t* A, const uint32_t* B, size_t n, uint32_t* native_proof, uint32_t* statement, int* accepted,
                 Lists& l) {
    if (sipp_native_proof_words(n) == 0) return sipp_prove_native_ex(ctx, A, B, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    try {
        l.size_for(n);
    } catch (const std::bad_alloc&) {
        return SIPP_E_NOMEM;
    }
    return sipp_prove_native_ex(ctx, A, B, n, native_proof, statement, l.rec[0].data(), l.rec[1].data(), l.rec[2].data(), accepted);
}

int stark_stage(sipp_ctx* const ctxs[3], const Lists& l, uint64_t* const proof_out[3], const size_t proof_cap[3], size_t proof_len[3]) {
    const uint32_t* ios[3] = {l.rec[0].data(), l.rec[1].data(), l.rec[2].data()};
    return sipp_instance_prove(ctxs, ios, l.num, proof_out, proof_cap, proof_len);
}

}  // namespace

extern "C" {

int sipp_flow_prove(sipp_ctx* native_ctx, sipp_ctx* const ctxs[3], const uint32_t* A, const uint32_t* B, size_t n, uint32_t* native_proof,
                    uint32_t* statement, uint64_t* const proof_out[3], const size_t proof_cap[3], size_t proof_len[3], int* accepted) {
    if (!native_ctx || !ctxs || !A || !B || !proof_out || !proof_cap || !proof_len) return SIPP_E_BADARG;
    for (int k = 0; k < 3; k++)
        if (!ctxs[k]) return SIPP_E_BADARG;
    for (int k = 0; k < 3; k++) proof_len[k] = 0;
    Lists l;
    const int rc = native_stage(native_ctx, A, B, n, native_proof, statement, accepted, l);
    if (rc != SIPP_OK) return rc;
    return stark_stage(ctxs, l, proof_out, proof_cap, proof_len);
}

int sipp_flows_prove(sipp_ctx* native_ctx, sipp_ctx* const* ctxs, size_t in_flight, size_t count, size_t n, const uint32_t* const* A,
                     const uint32_t* const* B, uint32_t* const* native_proof, uint32_t* const* statement, uint64_t* const* proof_out,
                     const size_t* proof_cap, size_t* proof_len, int* accepted, int* status) {
    if (!native_ctx || !ctxs || !in_flight) return SIPP_E_BADARG;
    for (size_t i = 0; i < 3 * in_flight; i++) {
        if (!ctxs[i] || ctxs[i] == native_ctx) return SIPP_E_BADARG;  // the producer's ctx works beside every slot
        for (size_t j = 0; j < i; j++)
            if (ctxs[i] == ctxs[j]) return SIPP_E_BADARG;
    }
    if (count == 0) return SIPP_OK;
    if (!A || !B || !proof_out || !proof_cap || !proof_len) return SIPP_E_BADARG;
    for (size_t i = 0; i < count; i++)
        if (!A[i] || !B[i]) return SIPP_E_BADARG;
    if (n > 1)
        for (size_t i = 0; i < 3 * count; i++)
            if (!proof_out[i]) return SIPP_E_BADARG;  // n = 1 has no obligation: no proof, no buffer
    for (size_t i = 0; i < 3 * count; i++) proof_len[i] = 0;

    // instance i: PENDING until the producer has run its native stage, then READY (its lists exist) or REFUSED (rcs[i] says why)
    enum { PENDING, READY, REFUSED };
    std::vector<Lists> lists;
    std::vector<int> state, rcs;
    try {
        lists.resize(count);
        state.assign(count, PENDING);
        rcs.assign(count, SIPP_OK);
    } catch (const std::bad_alloc&) {
        return SIPP_E_NOMEM;
    }
    std::mutex mu;
    std::condition_variable cv;
    size_t next = 0;  // the next instance a slot takes (under mu)

    auto producer = [&]() {
        for (size_t i = 0; i < count; i++) {
            int rc;
            try {
                rc = native_stage(native_ctx, A[i], B[i], n, native_proof ? native_proof[i] : nullptr, statement ? statement[i] : nullptr,
                                  accepted ? &accepted[i] : nullptr, lists[i]);
            } catch (...) {
                rc = SIPP_E_NOMEM;
            }
            std::lock_guard<std::mutex> lk(mu);
            rcs[i] = rc;
            state[i] = rc == SIPP_OK ? READY : REFUSED;
            cv.notify_all();
        }
    };
    auto worker = [&](size_t slot) {
        for (;;) {
            size_t i;
            {
                std::unique_lock<std::mutex> lk(mu);
                i = next++;
                if (i >= count) return;
                // the producer settles every instance before it returns (above: no path leaves the loop early), so this wait ends
                cv.wait(lk, [&] { return state[i] != PENDING; });
                if (state[i] == REFUSED) continue;  // no proof is attempted for it
            }
            const int rc = stark_stage(ctxs + 3 * slot, lists[i], proof_out + 3 * i, proof_cap + 3 * i, proof_len + 3 * i);
            lists[i] = Lists();  // the lists of a proved instance are not kept
            std::lock_guard<std::mutex> lk(mu);
            rcs[i] = rc;
        }
    };
    // no exception may cross the C ABI, and a joinable std::thread must not be destroyed.  If the producer's thread cannot be created
    // the native stages run here first, one after the other; if a slot's thread cannot be created, the slots that did start plus this
    // thread drain the queue -- fewer threads, same result
    std::thread prod;
    bool prod_started = false;
    try {
        prod = std::thread(producer);
        prod_started = true;
    } catch (...) {
    }
    if (!prod_started) producer();
    std::vector<std::thread> pool;
    const size_t slots = in_flight < count ? in_flight : count;
    try {
        pool.reserve(slots);
        for (size_t sl = 1; sl < slots; sl++) pool.emplace_back(worker, sl);
    } catch (...) {
    }
    worker(0);
    for (auto& t : pool) t.join();
    if (prod_started) prod.join();
    int first_rc = SIPP_OK;  // the first failing status by instance index
    for (size_t i = 0; i < count; i++) {
        if (status) status[i] = rcs[i];
        if (rcs[i] != SIPP_OK && first_rc == SIPP_OK) first_rc = rcs[i];
    }
    return first_rc;
}

}  // extern "C"
