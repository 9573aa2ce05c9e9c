"""ctypes binding of include/sipp_hip.h -- the same surface a Rust `extern "C"` block would bind
(INTEGRATION.md).  Device memory is plain torch tensors (dtype int64 viewed as u64)."""
import ctypes as C
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libsipp_hip.so")

P = 2**64 - 2**32 + 1

STATUS = {
    0: "SIPP_OK", -1: "SIPP_E_BADARG", -2: "SIPP_E_HIP", -3: "SIPP_E_NOMEM", -4: "SIPP_E_BUFSZ",
    -5: "SIPP_E_SUBGROUP", -6: "SIPP_E_QUOTIENT", -7: "SIPP_E_UNSUPPORTED", -8: "SIPP_E_WITNESS", -9: "SIPP_E_VERIFY",
}


class SippError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d): %s" % (STATUS.get(code, "?"), code, msg))
        self.code = code


class StarkConfig(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("rate_bits", "cap_height", "pow_bits", "arity_bits", "final_poly_bits",
                                          "num_queries", "num_challenges", "pow_rule", "fs_rule", "lookup_rule")]


class FriParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("rate_bits", "cap_height", "pow_bits", "num_queries", "pow_rule", "hiding", "n_rounds")] + \
               [("arity_bits", C.c_uint32 * 32)]


class Oracle(C.Structure):
    _fields_ = [("d_coeffs", C.c_void_p), ("d_lde", C.c_void_p), ("d_tree", C.c_void_p), ("n_polys", C.c_uint32), ("n_salt", C.c_uint32)]


class PolyRange(C.Structure):
    _fields_ = [("oracle", C.c_uint32), ("col_begin", C.c_uint32), ("col_end", C.c_uint32)]


class FriBatch(C.Structure):
    _fields_ = [("point", C.c_uint64 * 2), ("n_ranges", C.c_uint32), ("ranges", C.POINTER(PolyRange))]


class PlonkParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("num_routed_wires", "max_degree", "num_challenges")]


class PlonkGate(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("selector_index", "row", "group_lo", "group_hi", "prog_offset", "num_constraints")]


class PlonkCircuit(C.Structure):
    """sipp_plonk_circuit: the gate set as data (include/sipp_hip.h, "gates as data")"""
    _fields_ = [("num_wires", C.c_uint32), ("num_constants", C.c_uint32), ("num_selectors", C.c_uint32), ("num_gates", C.c_uint32),
                ("gates", C.POINTER(PlonkGate)), ("programs", C.POINTER(C.c_int64)), ("program_words", C.c_uint32)]

    @classmethod
    def from_dict(cls, circ):
        """circ: dict(num_wires, num_constants, num_selectors, gates=[(selector_index, row, lo, hi, prog_offset, n_constraints)], programs)"""
        gates = (PlonkGate * len(circ["gates"]))(*[PlonkGate(*[int(x) for x in g]) for g in circ["gates"]])
        prog = np.ascontiguousarray(circ["programs"], dtype=np.int64)
        c = cls(circ["num_wires"], circ["num_constants"], circ["num_selectors"], len(circ["gates"]), gates,
                prog.ctypes.data_as(C.POINTER(C.c_int64)), len(prog))
        c._keep = (gates, prog)           # the struct points into these
        return c


# include/sipp_hip.h SIPP_GEN_*: the u32 and nonnative families (sipp_amd/nonnative.py builds on them)
GEN_U32_ARITHMETIC, GEN_U32_ADD_MANY, GEN_NONNATIVE = 19, 20, 21


class PlonkGenerator(C.Structure):
    """sipp_plonk_generator: one gate family's witness generator with its layout (include/sipp_hip.h, "WITNESS GENERATORS")"""
    _fields_ = [("kind", C.c_uint32), ("selector_index", C.c_uint32), ("row", C.c_uint32), ("p", C.c_uint32 * 5)]


def _gen_array(gens):
    """gens = [(kind, selector_index, row, p0 .. p4)] as the array the C calls take (one unused element for an empty list)"""
    return (PlonkGenerator * max(1, len(gens)))(*[PlonkGenerator(int(g[0]), int(g[1]), int(g[2]), (C.c_uint32 * 5)(*[int(x) for x in g[3:8]])) for g in gens])


class PlonkSchedule(C.Structure):
    """sipp_plonk_schedule: rows sorted by level + the copies each level's outputs feed (include/sipp_hip.h)"""
    _fields_ = [("n_levels", C.c_uint32), ("d_rows", C.c_void_p), ("level_offsets", C.POINTER(C.c_uint32)), ("d_copy_src", C.c_void_p),
                ("d_copy_dst", C.c_void_p), ("copy_offsets", C.POINTER(C.c_uint32))]

    @classmethod
    def from_dict(cls, sched):
        """sched: tools/plonk_synth.chain_schedule() -- uploads rows / copy cells, keeps the host offsets alive"""
        import torch
        rows = torch.from_numpy(np.ascontiguousarray(sched["rows"], dtype=np.uint32).view(np.int32)).cuda()
        src = to_device(np.ascontiguousarray(sched["copy_src"] if len(sched["copy_src"]) else [0], dtype=np.uint64))
        dst = to_device(np.ascontiguousarray(sched["copy_dst"] if len(sched["copy_dst"]) else [0], dtype=np.uint64))
        lo = np.ascontiguousarray(sched["level_offsets"], dtype=np.uint32)
        co = np.ascontiguousarray(sched["copy_offsets"], dtype=np.uint32)
        s = cls(int(sched["n_levels"]), rows.data_ptr(), lo.ctypes.data_as(C.POINTER(C.c_uint32)), src.data_ptr(), dst.data_ptr(),
                co.ctypes.data_as(C.POINTER(C.c_uint32)))
        s._keep = (rows, src, dst, lo, co)
        return s


class PlonkScheduleHost(C.Structure):
    """sipp_plonk_schedule_host: the level schedule as host arrays (sipp_circuit_build copies them)"""
    _fields_ = [("n_levels", C.c_uint32), ("rows", C.POINTER(C.c_uint32)), ("level_offsets", C.POINTER(C.c_uint32)), ("copy_src", C.POINTER(C.c_uint64)),
                ("copy_dst", C.POINTER(C.c_uint64)), ("copy_offsets", C.POINTER(C.c_uint32))]

    @classmethod
    def from_dict(cls, sched):
        a32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)
        a64 = lambda v: np.ascontiguousarray(v if len(v) else [0], dtype=np.uint64)
        keep = (a32(sched["rows"]), a32(sched["level_offsets"]), a64(sched["copy_src"]), a64(sched["copy_dst"]), a32(sched["copy_offsets"]))
        p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        s = cls(int(sched["n_levels"]), keep[0].ctypes.data_as(p32), keep[1].ctypes.data_as(p32), keep[2].ctypes.data_as(p64),
                keep[3].ctypes.data_as(p64), keep[4].ctypes.data_as(p32))
        s._keep = keep
        return s


class Blinding(C.Structure):
    """sipp_blinding: the seed of a zero-knowledge prover (four canonical words, secret) and the number of the proof under it; the C
    calls take its five words (C.byref of one)"""
    _fields_ = [("seed", C.c_uint64 * 4), ("counter", C.c_uint64)]

    @classmethod
    def of(cls, seed, counter=0):
        return cls((C.c_uint64 * 4)(*[int(x) for x in seed]), int(counter))


class Challenger(C.Structure):
    _fields_ = [("state", C.c_uint64 * 12), ("in_buf", C.c_uint64 * 8), ("n_in", C.c_uint64), ("out_buf", C.c_uint64 * 8),
                ("n_out", C.c_uint64)]


# every symbol include/sipp_hip.h declares: name -> (restype, argtypes)
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
vp = C.c_void_p
SIGNATURES = {
    "sipp_default_config": (None, [C.POINTER(StarkConfig)]),
    "sipp_ctx_create": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(StarkConfig), C.c_size_t]),
    "sipp_ctx_destroy": (None, [vp]),
    "sipp_abi_version": (C.c_uint32, []),
    "sipp_ctx_create_checked": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(StarkConfig), C.c_size_t, C.c_uint32, C.c_size_t]),
    "sipp_ctx_set_kernel_routes": (C.c_int, [vp, C.c_uint32]),
    "sipp_ctx_set_stream_priority": (C.c_int, [vp, C.c_int]),
    "sipp_last_error": (C.c_char_p, [vp]),
    "sipp_sync": (C.c_int, [vp]),
    "sipp_stream": (vp, [vp]),
    "sipp_g1_exp_prove": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_g2_exp_prove": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_fq12_exp_prove": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_map_to_g2_prove": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_pairing_prove": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_prove": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_ctx_set_hardened": (C.c_int, [vp, C.c_int]),
    "sipp_map_to_g2": (C.c_int, [vp, vp, C.c_size_t, vp, vp, vp]),
    "sipp_prove_async": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t]),
    "sipp_wait": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "sipp_host_poseidon_permute": (C.c_int, [vp, C.c_size_t, C.c_int]),
    "sipp_instances_prove": (C.c_int, [C.POINTER(vp), C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "sipp_io_shard": (C.c_int, [C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sipp_instance_prove": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sipp_exp_outputs": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "sipp_inner_product": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "sipp_inner_products": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, vp]),
    "sipp_native_proof_words": (C.c_size_t, [C.c_size_t]),
    "sipp_prove_native": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "sipp_verify_native": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
    "sipp_prove_native_ex": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
    "sipp_flow_prove": (C.c_int, [vp, C.POINTER(vp), vp, vp, C.c_size_t, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                  C.POINTER(C.c_int)]),
    "sipp_flows_prove": (C.c_int, [vp, C.POINTER(vp), C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                   C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "sipp_stark_verify": (C.c_int, [u64p, C.c_size_t, C.POINTER(StarkConfig), C.POINTER(C.c_int)]),
    "sipp_fri_verify_openings": (C.c_int, [u64p, C.c_size_t, C.POINTER(u64p), u32p, u32p, C.c_size_t, C.POINTER(FriBatch), C.c_size_t, C.c_uint32,
                                           C.POINTER(FriParams), C.POINTER(Challenger), C.POINTER(C.c_int)]),
    "sipp_plonk_verify_gates": (C.c_int, [u64p, C.c_size_t, u64p, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p,
                                          C.POINTER(C.c_int)]),
    "sipp_proof_size": (C.c_size_t, [vp, C.c_int, C.c_size_t]),
    "sipp_stark_shape": (C.c_int, [vp, C.c_int, C.c_size_t, u32p, u32p, u32p, u32p]),
    "sipp_workspace_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "sipp_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sipp_workspace_bytes_cfg": (C.c_size_t, [C.c_int, C.c_size_t, C.POINTER(StarkConfig)]),
    "sipp_fri_const_arity": (None, [C.POINTER(FriParams), C.c_uint32, C.c_uint32, C.c_uint32]),
    "sipp_commit_batch_ex": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp]),
    "sipp_fri_proof_size": (C.c_size_t, [C.POINTER(Oracle), C.c_size_t, C.POINTER(FriBatch), C.c_size_t, C.c_uint32, C.POINTER(FriParams)]),
    "sipp_fri_prove_openings": (C.c_int, [vp, C.POINTER(Oracle), C.c_size_t, C.POINTER(FriBatch), C.c_size_t, C.c_uint32,
                                          C.POINTER(FriParams), C.POINTER(Challenger), vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_plonk_num_partial_products": (C.c_uint32, [C.POINTER(PlonkParams)]),
    "sipp_plonk_zs_partial_products": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(PlonkParams), u64p, u64p, vp]),
    "sipp_plonk_lookup_num_columns": (C.c_uint32, [C.POINTER(PlonkParams), u32p]),
    "sipp_plonk_lookup_multiplicities": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
    "sipp_plonk_lookup_sums": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlonkParams), u32p, u64p, u64p, vp]),
    "sipp_plonk_quotient_chunks": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(PlonkParams), u64p, u64p, u64p, vp]),
    "sipp_plonk_quotient_chunks_ex": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(PlonkParams), u64p, u64p, u64p, vp, C.c_uint32, vp]),
    "sipp_plonk_prove_ex": (C.c_int, [vp, vp, vp, C.POINTER(Oracle), u64p, C.POINTER(Oracle), C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams),
                                      u64p, u64p, C.c_uint32, vp, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_plonk_perm_proof_size": (C.c_size_t, [C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams)]),
    "sipp_plonk_gates_proof_size": (C.c_size_t, [C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), C.c_uint32]),
    "sipp_plonk_prove_gates": (C.c_int, [vp, vp, vp, C.POINTER(Oracle), u64p, C.POINTER(Oracle), C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams),
                                         C.POINTER(PlonkCircuit), u64p, u64p, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_plonk_gates_lookup_proof_size": (C.c_size_t, [C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), C.c_uint32,
                                                        u32p]),
    "sipp_plonk_prove_gates_lookup": (C.c_int, [vp, vp, vp, C.POINTER(Oracle), u64p, C.POINTER(Oracle), C.c_uint32, C.POINTER(PlonkParams),
                                                C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p, u64p, C.c_uint32, u32p, vp, C.c_size_t,
                                                C.POINTER(C.c_size_t)]),
    "sipp_plonk_verify_gates_lookup": (C.c_int, [u64p, C.c_size_t, u64p, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p,
                                                 u32p, C.POINTER(C.c_int)]),
    "sipp_circuit_set_lookup": (C.c_int, [vp, u32p]),
    "sipp_blind_salt": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32]),
    "sipp_plonk_gates_zk_proof_size": (C.c_size_t, [C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), C.c_uint32,
                                                    u32p]),
    "sipp_plonk_prove_gates_zk": (C.c_int, [vp, vp, vp, C.POINTER(Oracle), u64p, C.POINTER(Oracle), C.c_uint32, C.POINTER(PlonkParams),
                                            C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p, u64p, C.c_uint32, u32p, vp, vp,
                                            C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_circuit_set_blinding": (C.c_int, [vp, u64p]),
    "sipp_plonk_generate_witness_blind": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlonkGenerator), C.c_size_t, u64p,
                                                    vp]),
    "sipp_plonk_generate_witness_levels_blind": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlonkGenerator), C.c_size_t,
                                                           u64p, C.POINTER(PlonkSchedule), vp]),
    "sipp_plonk_generate_witness": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlonkGenerator), C.c_size_t, u64p]),
    "sipp_plonk_generate_witness_levels": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PlonkGenerator), C.c_size_t, u64p,
                                                     C.POINTER(PlonkSchedule)]),
    "sipp_circuit_workspace_bytes": (C.c_size_t, [C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit)]),
    "sipp_circuit_build": (C.c_int, [vp, C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), vp, C.POINTER(PlonkGenerator),
                                     C.c_size_t, C.POINTER(PlonkScheduleHost), u64p, C.POINTER(vp)]),
    "sipp_circuit_destroy": (None, [vp]),
    "sipp_circuit_verifier_data": (C.c_int, [vp, vp, vp]),
    "sipp_circuit_proof_size": (C.c_size_t, [vp, C.c_uint32]),
    "sipp_circuit_prove": (C.c_int, [vp, vp, u64p, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_circuit_prove_inputs": (C.c_int, [vp, vp, vp, C.c_size_t, u64p, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_circuit_set_input_map": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t]),
    "sipp_circuit_prove_words": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, u64p, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_circuit_verify": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_int)]),
    "sipp_plonk_perm_prove": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), u64p, u64p, vp, C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    # the tree hasher as an argument (Keccak-256 Merkle trees)
    "sipp_merkle_leaves_h": (C.c_int, [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]),
    "sipp_merkle_levels_h": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    "sipp_fri_leaves_h": (C.c_int, [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]),
    "sipp_host_keccak256": (C.c_int, [vp, C.c_size_t, vp]),
    "sipp_host_merkle_hash": (C.c_int, [C.c_uint32, u64p, C.c_size_t, u64p, u64p]),
    "sipp_commit_batch_h": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp]),
    "sipp_fri_prove_openings_h": (C.c_int, [vp, C.POINTER(Oracle), C.c_size_t, C.POINTER(FriBatch), C.c_size_t, C.c_uint32,
                                            C.POINTER(FriParams), C.c_uint32, C.POINTER(Challenger), vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_fri_verify_openings_h": (C.c_int, [u64p, C.c_size_t, C.POINTER(u64p), u32p, u32p, C.c_size_t, C.POINTER(FriBatch), C.c_size_t, C.c_uint32,
                                             C.POINTER(FriParams), C.c_uint32, C.POINTER(Challenger), C.POINTER(C.c_int)]),
    "sipp_plonk_prove_gates_h": (C.c_int, [vp, vp, vp, C.POINTER(Oracle), u64p, C.POINTER(Oracle), C.c_uint32, C.POINTER(PlonkParams),
                                           C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p, u64p, C.c_uint32, u32p, vp, C.c_uint32, vp,
                                           C.c_size_t, C.POINTER(C.c_size_t)]),
    "sipp_plonk_verify_gates_h": (C.c_int, [u64p, C.c_size_t, u64p, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), u64p,
                                            u32p, C.c_uint32, C.POINTER(C.c_int)]),
    "sipp_circuit_build_h": (C.c_int, [vp, C.c_uint32, C.POINTER(PlonkParams), C.POINTER(FriParams), C.POINTER(PlonkCircuit), vp,
                                       C.POINTER(PlonkGenerator), C.c_size_t, C.POINTER(PlonkScheduleHost), u64p, C.c_uint32, C.POINTER(vp)]),
    "sipp_ntt_batch": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.c_uint32, C.c_int]),
    "sipp_lde_batch": (C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_uint32]),
    "sipp_poseidon_leaves": (C.c_int, [vp, vp, C.c_size_t, C.c_uint32, vp]),
    "sipp_merkle_cap": (C.c_int, [vp, vp, C.c_uint32, vp]),
    "sipp_commit_batch": (C.c_int, [vp, vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp]),
    "sipp_poseidon_permute": (C.c_int, [vp, vp, C.c_size_t]),
    "sipp_trace_build": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp]),
    "sipp_profile_enable": (C.c_int, [vp, C.c_int]),
    "sipp_profile_reset": (C.c_int, [vp]),
    "sipp_profile_report": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "sipp_timer_start": (C.c_int, [vp]),
    "sipp_timer_stop": (C.c_int, [vp, C.POINTER(C.c_float)]),
}

_lib = None


def lib():
    """Load libsipp_hip.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        raise SippError(-7, "libsipp_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # torch ships its own libamdhip64: load torch FIRST so that libsipp_hip.so binds to the same HIP runtime
    # (two runtimes in one process make hipGetDeviceCount fail in whichever comes second)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(SO)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


SIPP_E_VERIFY = -9
# the tree hasher of the _h entries (include/sipp_hip.h): Poseidon, or Keccak-256 truncated to 25 bytes (plonky2's KeccakGoldilocksConfig)
HASH_POSEIDON, HASH_KECCAK25 = 0, 1
HASHERS = {"poseidon": HASH_POSEIDON, "keccak": HASH_KECCAK25}
PLONK_HEADER_HASHER_WORD = 13      # of a flat "SIPPPLK3/4/5" proof: 0 under Poseidon, as it always was


def hasher_id(hasher):
    """'poseidon' / 'keccak' (or the number itself) -> the uint32 the C calls take; anything else ValueError"""
    if isinstance(hasher, str):
        if hasher not in HASHERS:
            raise ValueError("hasher must be 'poseidon' or 'keccak', not %r" % (hasher,))
        return HASHERS[hasher]
    return int(hasher)


def plonk_proof_hasher(proof):
    """the tree hasher a flat "SIPPPLK3/4/5" proof names in its header"""
    return int(np.asarray(proof, dtype=np.uint64)[PLONK_HEADER_HASHER_WORD])


def refuse_keccak_proof(proof, who):
    """the recursion circuits verify Poseidon trees only: a proof whose header names another hasher is refused before anything is launched"""
    pf = np.asarray(proof, dtype=np.uint64).reshape(-1)
    if len(pf) > PLONK_HEADER_HASHER_WORD and int(pf[PLONK_HEADER_HASHER_WORD]) != HASH_POSEIDON:
        raise ValueError("%s: the proof's Merkle trees are hashed with hasher %d (header word %d); the circuit verifies Poseidon trees only"
                         % (who, int(pf[PLONK_HEADER_HASHER_WORD]), PLONK_HEADER_HASHER_WORD))


def host_keccak256(data):
    """sipp_host_keccak256: Keccak-256 (original padding) of a bytes object on the host -> 32 bytes"""
    data = bytes(data)
    out = C.create_string_buffer(32)
    rc = lib().sipp_host_keccak256(C.c_char_p(data) if data else None, len(data), out)
    if rc:
        raise SippError(rc, "sipp_host_keccak256")
    return out.raw


def host_merkle_hash(hasher, elements, right=None):
    """sipp_host_merkle_hash: the host verifier's hash_or_noop(elements), or two_to_one(elements, right) of two digests -> four words"""
    e = np.ascontiguousarray(elements, dtype=np.uint64).reshape(-1)
    r = None if right is None else np.ascontiguousarray(right, dtype=np.uint64).reshape(-1)
    out = np.zeros(4, dtype=np.uint64)
    rc = lib().sipp_host_merkle_hash(hasher_id(hasher), e.ctypes.data_as(u64p) if len(e) else None, len(e),
                                     None if r is None else r.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
    if rc:
        raise SippError(rc, "sipp_host_merkle_hash")
    return out


def _verify_gates(name, proof, constants_sigmas_cap, p, fp, circuit, digest, extra):
    """what plonk_verify_gates_lookup / _h share: the call `name` with `extra` between the digest and the reason -> 0 or the refusing stage"""
    pf = np.ascontiguousarray(proof, dtype=np.uint64)
    cap = np.ascontiguousarray(constants_sigmas_cap, dtype=np.uint64).reshape(-1)
    reason = C.c_int(0)
    rc = getattr(lib(), name)(pf.ctypes.data_as(u64p), len(pf), cap.ctypes.data_as(u64p), C.byref(p), C.byref(fp), C.byref(circuit),
                              (C.c_uint64 * 4)(*[int(x) for x in digest]), *extra, C.byref(reason))
    if rc not in (0, SIPP_E_VERIFY):
        raise SippError(rc, name)
    return reason.value


def plonk_verify_gates_h(proof, constants_sigmas_cap, p, fp, circuit, digest, lookup, hasher):
    """sipp_plonk_verify_gates_h: plonk_verify_gates_lookup (lookup may be None) with the tree hasher.  Returns 0 or the refusing stage."""
    return _verify_gates("sipp_plonk_verify_gates_h", proof, constants_sigmas_cap, p, fp, circuit, digest,
                         [None if lookup is None else Ctx._lookup_words(lookup), hasher_id(hasher)])


def fri_verify_openings_h(proof, caps, ncols, n_salt, batches, log_n, params, challenger, hasher):
    """sipp_fri_verify_openings_h: caps = one array per oracle, batches as Ctx.fri_prove_openings takes them; `challenger` is advanced in
    place.  Returns 0 or the refusing stage."""
    pf = np.ascontiguousarray(proof, dtype=np.uint64)
    keep = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in caps]
    cp = (u64p * len(keep))(*[k.ctypes.data_as(u64p) for k in keep])
    ba, keep2 = Ctx._batches(batches)
    reason = C.c_int(0)
    rc = lib().sipp_fri_verify_openings_h(pf.ctypes.data_as(u64p), len(pf), cp, (C.c_uint32 * len(keep))(*[int(x) for x in ncols]),
                                          (C.c_uint32 * len(keep))(*[int(x) for x in n_salt]), len(keep), ba, len(batches), log_n,
                                          C.byref(params), hasher_id(hasher), C.byref(challenger), C.byref(reason))
    if rc not in (0, SIPP_E_VERIFY):
        raise SippError(rc, "sipp_fri_verify_openings_h")
    return reason.value


def plonk_verify_gates_lookup(proof, constants_sigmas_cap, p, fp, circuit, digest, lookup):
    """sipp_plonk_verify_gates_lookup: the library's own check of a "SIPPPLK4" proof (host code; no ctx, no GPU) against the caller's
    lookup description (eight words; an empty one: a "SIPPPLK3" proof).  Under fp.hiding = 1 it accepts a "SIPPPLK5" proof alone, under
    hiding = 0 none.  Returns 0 for an accepted proof, else the refusing stage."""
    return _verify_gates("sipp_plonk_verify_gates_lookup", proof, constants_sigmas_cap, p, fp, circuit, digest, [Ctx._lookup_words(lookup)])


def stark_verify(proof, cfg=None):
    """sipp_stark_verify: the library's own check of a flat proof (host code; no ctx, no GPU).  Returns 0 for an accepted proof, else the
    stage that refused it (include/sipp_hip.h lists them: 110 = the constraints do not meet the quotient, 123 = a Merkle path ...).
    Raises SippError for a call the library cannot serve (SIPP_E_BADARG / SIPP_E_UNSUPPORTED)."""
    pf = np.ascontiguousarray(proof, dtype=np.uint64)
    reason = C.c_int(0)
    rc = lib().sipp_stark_verify(pf.ctypes.data_as(u64p), len(pf), C.byref(cfg) if cfg is not None else None, C.byref(reason))
    if rc not in (0, SIPP_E_VERIFY):
        raise SippError(rc, "sipp_stark_verify")
    return reason.value


def default_config():
    cfg = StarkConfig()
    lib().sipp_default_config(C.byref(cfg))
    return cfg


def device_memory_bytes(device=0):
    """total memory of GPU `device` (sipp_device_memory)"""
    total = C.c_size_t()
    rc = lib().sipp_device_memory(int(device), None, C.byref(total))
    if rc != 0:
        raise SippError(rc, "device_memory")
    return total.value


def device_free_bytes(device=0):
    """free memory of GPU `device` right now (sipp_device_memory)"""
    free = C.c_size_t()
    rc = lib().sipp_device_memory(int(device), C.byref(free), None)
    if rc != 0:
        raise SippError(rc, "device_memory")
    return free.value


def to_device(arr):
    """host uint64 ndarray -> device tensor (int64 bit pattern)"""
    import torch
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to("cuda")


def to_host(t):
    return t.detach().cpu().numpy().view(np.uint64)


def native_points(A, B, what="native"):
    """the points of one SIPP instance as the native chain takes them: A [n, 16], B [n, 32] uint32 limbs, n a power of two ->
    (A, B, n, log2 n); SippError(SIPP_E_BADARG) for anything else, before any call into the library"""
    A = np.ascontiguousarray(A, dtype=np.uint32)
    B = np.ascontiguousarray(B, dtype=np.uint32)
    if A.size == 0 or A.size % 16 or B.size % 32:
        raise SippError(-1, "%s: A must be [n, 16] and B [n, 32] uint32 limbs" % what)
    A, B = A.reshape(-1, 16), B.reshape(-1, 32)
    n = A.shape[0]
    if B.shape[0] != n or n & (n - 1):
        raise SippError(-1, "%s: |A| = |B| = n must be a power of two" % what)
    return A, B, n, n.bit_length() - 1


def native_output_shapes(n):
    """shapes of what the native chain returns for n pairs (include/sipp_hip.h): proof, statement, the three obligation lists"""
    lg = n.bit_length() - 1
    return {"proof": (2 * lg + 1, 96), "statement": (48 * n + 240,), "g1": (n - 1, 56), "g2": (n - 1, 104), "fq12": (2 * lg, 296)}


def _native_out(out, key, shape, what):
    """the caller's array for output `key` (C-contiguous uint32 of exactly `shape`) or a fresh zeroed one"""
    if out is None or key not in out:
        return np.zeros(shape, dtype=np.uint32)
    a = out[key]
    if not isinstance(a, np.ndarray) or a.dtype != np.uint32 or a.shape != tuple(shape) or not a.flags.c_contiguous or not a.flags.writeable:
        raise SippError(-1, "%s: out[%r] must be a writeable C-contiguous uint32 array of shape %r" % (what, key, tuple(shape)))
    return a


class Ctx:
    """One GPU, one stream, one workspace arena (sipp_ctx)."""

    def __init__(self, device=0, cfg=None, workspace_bytes=1 << 30):
        import torch
        if not torch.cuda.is_available():
            raise SippError(-2, "no GPU visible: the SIPP HIP path has no CPU fallback")
        self.L = lib()
        self.device = device
        torch.cuda.set_device(device)
        h = vp()
        rc = self.L.sipp_ctx_create(C.byref(h), device, C.byref(cfg) if cfg is not None else None, workspace_bytes)
        if rc != 0:
            raise SippError(rc, "sipp_ctx_create")
        self.h = h
        self.workspace_bytes = int(workspace_bytes) if workspace_bytes else 24 << 30      # the arena this ctx reserved (0 = the library's default)
        self.cfg = cfg if cfg is not None else default_config()

    def close(self):
        if getattr(self, "h", None):
            self.L.sipp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise SippError(rc, "%s: %s" % (what, self.L.sipp_last_error(self.h).decode()))

    def sync(self):
        self._ck(self.L.sipp_sync(self.h), "sync")

    # ---- building blocks (device tensors) ----
    def ntt(self, t, log_n, inverse=False):
        """in place, natural -> natural; t is [ncols, stride] int64"""
        assert t.is_cuda and t.dim() == 2 and t.is_contiguous()
        self._ck(self.L.sipp_ntt_batch(self.h, t.data_ptr(), t.shape[1], t.shape[0], log_n, int(inverse)), "ntt_batch")
        return t

    def lde(self, values, log_n):
        import torch
        ncols = values.shape[0]
        rb = self.cfg.rate_bits
        coeffs = torch.empty_like(values)
        lde = torch.empty((ncols, values.shape[1] << rb), dtype=torch.int64, device=values.device)
        self._ck(self.L.sipp_lde_batch(self.h, values.data_ptr(), coeffs.data_ptr(), lde.data_ptr(), ncols, log_n),
                 "lde_batch")
        return coeffs, lde

    def poseidon_leaves(self, lde, log_leaves):
        import torch
        dig = torch.empty(((1 << log_leaves), 4), dtype=torch.int64, device=lde.device)
        self._ck(self.L.sipp_poseidon_leaves(self.h, lde.data_ptr(), lde.shape[0], log_leaves, dig.data_ptr()),
                 "poseidon_leaves")
        return dig

    def merkle_cap(self, tree, log_leaves):
        ch = min(self.cfg.cap_height, log_leaves)
        cap = np.zeros((1 << ch, 4), dtype=np.uint64)
        self._ck(self.L.sipp_merkle_cap(self.h, tree.data_ptr(), log_leaves, cap.ctypes.data), "merkle_cap")
        return cap

    def merkle_leaves_h(self, lde, log_leaves, hasher):
        """sipp_merkle_leaves_h: lde [ncols, 2^log_leaves] device int64 (leaf order) -> digests [2^log_leaves, 4]"""
        import torch
        dig = torch.empty(((1 << log_leaves), 4), dtype=torch.int64, device=lde.device)
        self._ck(self.L.sipp_merkle_leaves_h(self.h, lde.data_ptr(), lde.shape[0], log_leaves, hasher_id(hasher), dig.data_ptr()), "merkle_leaves_h")
        return dig

    def merkle_levels_h(self, tree, log_leaves, cap_height, hasher):
        """sipp_merkle_levels_h: tree [2 << log_leaves, 4] device int64 with the leaf digests in front, completed in place -> the cap"""
        cap = np.zeros((1 << min(cap_height, log_leaves), 4), dtype=np.uint64)
        self._ck(self.L.sipp_merkle_levels_h(self.h, tree.data_ptr(), log_leaves, cap_height, hasher_id(hasher), cap.ctypes.data), "merkle_levels_h")
        return cap

    def fri_leaves_h(self, vals, arity_bits, hasher):
        """sipp_fri_leaves_h: vals [2, len] device int64 (c0 row, c1 row) -> digests [len >> arity_bits, 4]"""
        import torch
        dig = torch.empty((vals.shape[1] >> arity_bits, 4), dtype=torch.int64, device=vals.device)
        self._ck(self.L.sipp_fri_leaves_h(self.h, vals.data_ptr(), vals.shape[1], arity_bits, hasher_id(hasher), dig.data_ptr()), "fri_leaves_h")
        return dig

    def commit(self, values, log_n, bufs=None):
        """PolynomialBatch::from_values on device.  Returns (coeffs, lde, tree, cap)."""
        import torch
        ncols = values.shape[0]
        rb = self.cfg.rate_bits
        log_m = log_n + rb
        if bufs is None:
            coeffs = torch.empty_like(values)
            lde = torch.empty((ncols, 1 << log_m), dtype=torch.int64, device=values.device)
            tree = torch.empty((2 << log_m, 4), dtype=torch.int64, device=values.device)
        else:
            coeffs, lde, tree = bufs
        ch = min(self.cfg.cap_height, log_m)
        cap = np.zeros((1 << ch, 4), dtype=np.uint64)
        self._ck(self.L.sipp_commit_batch(self.h, values.data_ptr(), coeffs.data_ptr(), lde.data_ptr(),
                                          tree.data_ptr(), ncols, log_n, cap.ctypes.data), "commit_batch")
        return coeffs, lde, tree, cap

    # ---- generic PolynomialBatch / FRI opening proofs ----
    def commit_ex(self, data, log_n, rate_bits, cap_height, from_coeffs=False, salt=None, hasher=None):
        """sipp_commit_batch_ex: data [ncols, N] device int64 (values or coefficients), salt [4, N << rate_bits] or None.
        hasher: None = that call; 'poseidon' / 'keccak' = sipp_commit_batch_h.
        Returns (Oracle struct, cap ndarray, (coeffs, lde, tree) tensors kept alive by the caller)."""
        import torch
        ncols = data.shape[0]
        n_salt = 0 if salt is None else salt.shape[0]
        m = 1 << (log_n + rate_bits)
        coeffs = torch.empty_like(data)
        lde = torch.empty((ncols + n_salt, m), dtype=torch.int64, device=data.device)
        tree = torch.empty((2 * m, 4), dtype=torch.int64, device=data.device)
        ch = min(cap_height, log_n + rate_bits)
        cap = np.zeros((1 << ch, 4), dtype=np.uint64)
        head = [self.h, data.data_ptr(), int(from_coeffs), coeffs.data_ptr(), lde.data_ptr(), tree.data_ptr(), ncols, log_n, rate_bits, cap_height,
                None if salt is None else salt.data_ptr(), n_salt]
        if hasher is None:
            self._ck(self.L.sipp_commit_batch_ex(*head, cap.ctypes.data), "commit_batch_ex")
        else:
            self._ck(self.L.sipp_commit_batch_h(*head, hasher_id(hasher), cap.ctypes.data), "commit_batch_h")
        return Oracle(coeffs.data_ptr(), lde.data_ptr(), tree.data_ptr(), ncols, n_salt), cap, (coeffs, lde, tree)

    @staticmethod
    def _batches(batches):
        """[((c0, c1), [(oracle, col_begin, col_end), ...])] -> (FriBatch array, what must stay alive beside it)"""
        ba = (FriBatch * len(batches))()
        keep = []
        for i, (pt, ranges) in enumerate(batches):
            r = (PolyRange * len(ranges))(*[PolyRange(*x) for x in ranges])
            keep.append(r)
            ba[i].point[0], ba[i].point[1] = int(pt[0]), int(pt[1])
            ba[i].n_ranges = len(ranges)
            ba[i].ranges = r
        return ba, keep

    def fri_prove_openings(self, oracles, batches, log_n, params, challenger, hasher=None):
        """sipp_fri_prove_openings.  oracles: [Oracle], batches: [((c0, c1), [(oracle, col_begin, col_end), ...])];
        `challenger` (Challenger struct) is advanced in place.  hasher: None = that call; 'poseidon' / 'keccak' =
        sipp_fri_prove_openings_h (the oracles' trees committed with the same one).  Returns the flat proof."""
        oa = (Oracle * len(oracles))(*oracles)
        ba, keep = self._batches(batches)
        cap = self.L.sipp_fri_proof_size(oa, len(oracles), ba, len(batches), log_n, C.byref(params))
        if cap == 0:
            raise SippError(-1, "sipp_fri_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        if hasher is None:
            self._ck(self.L.sipp_fri_prove_openings(self.h, oa, len(oracles), ba, len(batches), log_n, C.byref(params),
                                                    C.byref(challenger), out.ctypes.data, cap, C.byref(n)), "fri_prove_openings")
        else:
            self._ck(self.L.sipp_fri_prove_openings_h(self.h, oa, len(oracles), ba, len(batches), log_n, C.byref(params), hasher_id(hasher),
                                                      C.byref(challenger), out.ctypes.data, cap, C.byref(n)), "fri_prove_openings_h")
        return out[: n.value]

    # ---- plonky2's wire permutation argument ----
    @staticmethod
    def _u64(v):
        a = (C.c_uint64 * len(v))(*[int(x) for x in v])
        return a

    def plonk_zs(self, wires, sigmas, log_n, p, betas, gammas):
        """sipp_plonk_zs_partial_products: wires, sigmas [R, N] device int64 -> [C (1 + num_prods), N]"""
        import torch
        rows = p.num_challenges * (1 + self.L.sipp_plonk_num_partial_products(C.byref(p)))
        out = torch.empty((rows, 1 << log_n), dtype=torch.int64, device=wires.device)
        self._ck(self.L.sipp_plonk_zs_partial_products(self.h, wires.data_ptr(), sigmas.data_ptr(), log_n, C.byref(p), self._u64(betas),
                                                       self._u64(gammas), out.data_ptr()), "plonk_zs_partial_products")
        return out

    # ---- lookup tables by a log-derivative argument (include/sipp_hip.h: the eight-word description) ----
    @staticmethod
    def _lookup_words(lookup):
        words = [int(x) for x in lookup]
        if len(words) != 8:
            raise SippError(-1, "a lookup description is eight words")
        return (C.c_uint32 * 8)(*words)

    def plonk_lookup_multiplicities(self, wires, constants, log_n, num_selectors, lookup):
        """sipp_plonk_lookup_multiplicities: wires [W, N], constants [K, N] device int64; the m cells of `wires` are rewritten in place"""
        assert wires.is_cuda and wires.is_contiguous() and constants.is_cuda and constants.is_contiguous()
        assert wires.shape[1] == constants.shape[1] == 1 << log_n
        self._ck(self.L.sipp_plonk_lookup_multiplicities(self.h, wires.data_ptr(), constants.data_ptr(), log_n, wires.shape[0],
                                                         constants.shape[0], num_selectors, self._lookup_words(lookup)),
                 "plonk_lookup_multiplicities")
        return wires

    def plonk_lookup_sums(self, wires, constants, log_n, num_selectors, p, lookup, etas, thetas):
        """sipp_plonk_lookup_sums: wires [W, N], constants [K, N] device int64 -> [C J, N]: S_0 .. S_(C-1), then the U's per challenge"""
        import torch
        assert wires.is_cuda and wires.is_contiguous() and constants.is_cuda and constants.is_contiguous()
        assert wires.shape[1] == constants.shape[1] == 1 << log_n
        words = self._lookup_words(lookup)
        rows = self.L.sipp_plonk_lookup_num_columns(C.byref(p), words)
        out = torch.empty((rows, 1 << log_n), dtype=torch.int64, device=wires.device)
        self._ck(self.L.sipp_plonk_lookup_sums(self.h, wires.data_ptr(), constants.data_ptr(), log_n, wires.shape[0], constants.shape[0],
                                               num_selectors, C.byref(p), words, self._u64(etas), self._u64(thetas), out.data_ptr()),
                 "plonk_lookup_sums")
        return out

    def plonk_quotient_chunks(self, wires_lde, sigmas_lde, zs_lde, log_n, rate_bits, p, betas, gammas, alphas):
        import torch
        out = torch.empty((p.num_challenges * p.max_degree, 1 << log_n), dtype=torch.int64, device=wires_lde.device)
        self._ck(self.L.sipp_plonk_quotient_chunks(self.h, wires_lde.data_ptr(), sigmas_lde.data_ptr(), zs_lde.data_ptr(), log_n, rate_bits,
                                                   C.byref(p), self._u64(betas), self._u64(gammas), self._u64(alphas), out.data_ptr()),
                 "plonk_quotient_chunks")
        return out

    def plonk_quotient_chunks_ex(self, wires_lde, sigmas_lde, zs_lde, log_n, rate_bits, p, betas, gammas, alphas, gate_terms):
        """gate_terms: [K, N << rate_bits] device int64 (leaf order) or None"""
        import torch
        out = torch.empty((p.num_challenges * p.max_degree, 1 << log_n), dtype=torch.int64, device=wires_lde.device)
        k = 0 if gate_terms is None else gate_terms.shape[0]
        self._ck(self.L.sipp_plonk_quotient_chunks_ex(self.h, wires_lde.data_ptr(), sigmas_lde.data_ptr(), zs_lde.data_ptr(), log_n, rate_bits,
                                                      C.byref(p), self._u64(betas), self._u64(gammas), self._u64(alphas),
                                                      None if gate_terms is None else gate_terms.data_ptr(), k, out.data_ptr()),
                 "plonk_quotient_chunks_ex")
        return out

    def _plonk_prove(self, fn, size_fn, cap, wires, second, wires_oracle, wires_cap, second_oracle, log_n, p, fp, circuit, digest, pis, extra):
        """what the three proof calls share: a buffer of `cap` words (the answer of `size_fn`; 0 = refused), the wires cap as an array
        that lives until the call returns, the call sipp_<fn> -- whose arguments differ in `circuit` (None: none) and in `extra`, the
        ones between the public inputs and the buffer -- and the proof cut to its length"""
        if cap == 0:
            raise SippError(-1, size_fn)
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        wc_arr = None if wires_cap is None else np.ascontiguousarray(wires_cap, dtype=np.uint64).reshape(-1)
        args = [self.h, wires.data_ptr(), second.data_ptr(), None if wires_oracle is None else C.byref(wires_oracle),
                None if wc_arr is None else wc_arr.ctypes.data_as(u64p), None if second_oracle is None else C.byref(second_oracle), log_n,
                C.byref(p), C.byref(fp)] + ([] if circuit is None else [C.byref(circuit)])
        args += [self._u64(digest), self._u64(pis) if pis else None, len(pis)] + list(extra) + [out.ctypes.data, cap, C.byref(n)]
        self._ck(getattr(self.L, "sipp_" + fn)(*args), fn)
        return out[: n.value]

    def plonk_prove_ex(self, wires, sigmas, log_n, p, fp, digest, public_inputs, gate_terms=None, wires_oracle=None, wires_cap=None,
                       sigmas_oracle=None):
        """sipp_plonk_prove_ex: the flow with gate terms, public inputs (host ints) and optional pre-committed oracles (Oracle structs)"""
        pis = [int(x) for x in public_inputs]
        cap = self.L.sipp_plonk_perm_proof_size(log_n, C.byref(p), C.byref(fp))
        extra = [None, 0] if gate_terms is None else [gate_terms.data_ptr(), gate_terms.shape[0]]
        return self._plonk_prove("plonk_prove_ex", "sipp_plonk_perm_proof_size", cap and cap + len(pis), wires, sigmas, wires_oracle, wires_cap,
                                 sigmas_oracle, log_n, p, fp, None, digest, pis, extra)

    def _prove_gates(self, fn, size_fn, size_extra, call_extra, wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs,
                     wires_oracle, wires_cap, cs_oracle):
        """the four gates-as-data calls: sipp_<size_fn>(.., n_public_inputs, *size_extra) sizes the buffer of sipp_<fn>(.., *call_extra, buffer)"""
        pis = [int(x) for x in public_inputs]
        cap = getattr(self.L, "sipp_" + size_fn)(log_n, C.byref(p), C.byref(fp), C.byref(circuit), len(pis), *size_extra)
        return self._plonk_prove(fn, "sipp_" + size_fn, cap, wires, constants_sigmas, wires_oracle, wires_cap, cs_oracle, log_n, p, fp, circuit,
                                 digest, pis, call_extra)

    def plonk_prove_gates(self, wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, wires_oracle=None, wires_cap=None,
                          cs_oracle=None):
        """sipp_plonk_prove_gates: wires [num_wires][N], constants_sigmas [num_constants + num_routed][N] device tensors (values);
        circuit = PlonkCircuit; the gate constraints are interpreted inside the quotient kernel.  Returns the flat "SIPPPLK3" proof."""
        return self._prove_gates("plonk_prove_gates", "plonk_gates_proof_size", [], [], wires, constants_sigmas, log_n, p, fp, circuit, digest,
                                 public_inputs, wires_oracle, wires_cap, cs_oracle)

    def plonk_prove_gates_lookup(self, wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, lookup, wires_oracle=None,
                                 wires_cap=None, cs_oracle=None):
        """sipp_plonk_prove_gates_lookup: plonk_prove_gates with a lookup description (eight words); the wire table holds the
        multiplicities already.  Returns the flat "SIPPPLK4" proof -- "SIPPPLK3", word for word plonk_prove_gates', for an empty one."""
        words = self._lookup_words(lookup)
        return self._prove_gates("plonk_prove_gates_lookup", "plonk_gates_lookup_proof_size", [words], [words], wires, constants_sigmas, log_n, p,
                                 fp, circuit, digest, public_inputs, wires_oracle, wires_cap, cs_oracle)

    def plonk_generate_witness(self, wires, constants, log_n, gens, pih=None, blind=None):
        """sipp_plonk_generate_witness: the gates' witness generators, in place on the device wire table [num_wires][N]; constants
        [>= num_constants][N] device tensor (the front of constants_sigmas); gens = [(kind, selector_index, row, p0 .. p4)];
        blind = Blinding (sipp_plonk_generate_witness_blind: what a SIPP_GEN_RANDOM generator needs) or None"""
        arr = _gen_array(gens)
        args = [self.h, wires.data_ptr(), constants.data_ptr(), log_n, wires.shape[0], constants.shape[0], arr, len(gens),
                None if pih is None else self._u64([int(x) for x in pih])]
        if blind is None:
            self._ck(self.L.sipp_plonk_generate_witness(*args), "plonk_generate_witness")
        else:
            self._ck(self.L.sipp_plonk_generate_witness_blind(*args, C.byref(blind)), "plonk_generate_witness_blind")

    def plonk_generate_witness_levels(self, wires, constants, log_n, gens, pih, sched, blind=None):
        """sipp_plonk_generate_witness_levels: the generators level by level with the copies between levels (sched = PlonkSchedule);
        synchronises the ctx stream (the schedule's bounds are checked on the device).  blind: as in plonk_generate_witness"""
        arr = _gen_array(gens)
        args = [self.h, wires.data_ptr(), constants.data_ptr(), log_n, wires.shape[0], constants.shape[0], arr, len(gens),
                None if pih is None else self._u64([int(x) for x in pih]), C.byref(sched)]
        if blind is None:
            self._ck(self.L.sipp_plonk_generate_witness_levels(*args), "plonk_generate_witness_levels")
        else:
            self._ck(self.L.sipp_plonk_generate_witness_levels_blind(*args, C.byref(blind)), "plonk_generate_witness_levels_blind")

    def plonk_prove_gates_zk(self, wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, lookup, blind, wires_oracle=None,
                             wires_cap=None, cs_oracle=None):
        """sipp_plonk_prove_gates_zk: plonk_prove_gates_lookup with blind = Blinding (fp.hiding = 1: salted wires, Z / partial-products
        and quotient oracles, the flat "SIPPPLK5" proof) or None (that call, byte for byte)"""
        words = self._lookup_words(lookup)
        return self._prove_gates("plonk_prove_gates_zk", "plonk_gates_zk_proof_size", [words], [words, None if blind is None else C.byref(blind)],
                                 wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, wires_oracle, wires_cap, cs_oracle)

    def plonk_prove_gates_h(self, wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, lookup, blind, hasher, wires_oracle=None,
                            wires_cap=None, cs_oracle=None):
        """sipp_plonk_prove_gates_h: plonk_prove_gates_zk (lookup and blind may each be None) with the tree hasher 'poseidon' / 'keccak';
        pre-committed oracles must have been committed with the same one.  The proof names the hasher in header word 13."""
        words = self._lookup_words(lookup if lookup is not None else (0,) * 8)
        return self._prove_gates("plonk_prove_gates_h", "plonk_gates_zk_proof_size", [words],
                                 [None if lookup is None else words, None if blind is None else C.byref(blind), hasher_id(hasher)],
                                 wires, constants_sigmas, log_n, p, fp, circuit, digest, public_inputs, wires_oracle, wires_cap, cs_oracle)

    def blind_salt(self, lde, ncols, log_m, blind, stream):
        """sipp_blind_salt: the four salt columns of stream 1 .. 3 behind the ncols polynomial columns of lde [ncols + 4, 2^log_m] (device
        int64, leaf order), in place"""
        assert lde.is_contiguous() and lde.shape[0] >= ncols + 4 and lde.shape[1] == 1 << log_m
        self._ck(self.L.sipp_blind_salt(self.h, lde.data_ptr(), ncols, log_m, C.byref(blind), stream), "blind_salt")

    def plonk_perm_prove(self, wires, sigmas, log_n, p, fp, digest=(1, 2, 3, 4), pih=(0, 0, 0, 0)):
        cap = self.L.sipp_plonk_perm_proof_size(log_n, C.byref(p), C.byref(fp))
        if cap == 0:
            raise SippError(-1, "sipp_plonk_perm_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        self._ck(self.L.sipp_plonk_perm_prove(self.h, wires.data_ptr(), sigmas.data_ptr(), log_n, C.byref(p), C.byref(fp), self._u64(digest),
                                              self._u64(pih), out.ctypes.data, cap, C.byref(n)), "plonk_perm_prove")
        return out[: n.value]

    def shape(self, kind, num_io):
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.sipp_stark_shape(self.h, kind, num_io, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "stark_shape")
        return a.value, b.value, c.value, d.value

    def trace_build(self, kind, ios):
        """device trace [W][N] (natural row order) for the IO records (host uint32 [num_io][words])"""
        import torch
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        log_n, W, _, _ = self.shape(kind, ios.shape[0])
        t = torch.empty((W, 1 << log_n), dtype=torch.int64, device="cuda")
        self._ck(self.L.sipp_trace_build(self.h, kind, ios.ctypes.data, ios.shape[0], t.data_ptr()), "trace_build")
        return t

    def prove(self, kind, ios):
        """one STARK sub-proof (kind 0 G1 / 1 G2 / 2 Fq12 / 3 MapToG2 / 4, 5 hardened G1, G2 / 6 final pairing) for host IO records -> flat proof"""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        cap = self.L.sipp_proof_size(self.h, kind, ios.shape[0])
        if cap == 0:
            raise SippError(-1, "sipp_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        if kind == 6:
            self._ck(self.L.sipp_pairing_prove(self.h, ios.ctypes.data, ios.shape[0], out.ctypes.data, cap, C.byref(n)), "pairing_prove")
            return out[: n.value]
        if kind >= 4:       # the hardened G1 / G2 kinds: the generic entry point
            self._ck(self.L.sipp_prove(self.h, kind, ios.ctypes.data, ios.shape[0], out.ctypes.data, cap, C.byref(n)), "prove")
            return out[: n.value]
        fn = (self.L.sipp_g1_exp_prove, self.L.sipp_g2_exp_prove, self.L.sipp_fq12_exp_prove, self.L.sipp_map_to_g2_prove)[kind]
        self._ck(fn(self.h, ios.ctypes.data, ios.shape[0], out.ctypes.data, cap, C.byref(n)), "prove")
        return out[: n.value]

    def exp_outputs(self, kind, ios):
        """copy of the records with the output words computed on the device (sipp_exp_outputs)"""
        rec = np.array(ios, dtype=np.uint32, order="C", copy=True)
        self._ck(self.L.sipp_exp_outputs(self.h, kind, rec.ctypes.data, rec.shape[0]), "exp_outputs")
        return rec

    def map_to_g2(self, msgs, cofactor=True):
        """messages [n][16] (u in Fp2) -> (MapToG2 records [n][48], G2ExpStark records of the cofactor clearing [2n][104],
        cleared points [n][32]) -- sipp_map_to_g2; without `cofactor` only the records"""
        msgs = np.ascontiguousarray(msgs, dtype=np.uint32).reshape(-1, 16)
        n = msgs.shape[0]
        recs = np.zeros((n, 48), dtype=np.uint32)
        if not cofactor:
            self._ck(self.L.sipp_map_to_g2(self.h, msgs.ctypes.data, n, recs.ctypes.data, None, None), "map_to_g2")
            return recs
        g2 = np.zeros((2 * n, 104), dtype=np.uint32)
        pts = np.zeros((n, 32), dtype=np.uint32)
        self._ck(self.L.sipp_map_to_g2(self.h, msgs.ctypes.data, n, recs.ctypes.data, g2.ctypes.data, pts.ctypes.data), "map_to_g2")
        return recs, g2, pts

    def inner_products(self, g1, g2, count=1):
        """prod_i pairing(A_i, B_i) (sipp_inner_products): g1 [count * n, 16], g2 [count * n, 32] uint32 limbs -> [count, 96]"""
        g1 = np.ascontiguousarray(g1, dtype=np.uint32).reshape(-1, 16)
        g2 = np.ascontiguousarray(g2, dtype=np.uint32).reshape(-1, 32)
        assert g1.shape[0] == g2.shape[0] and g1.shape[0] % count == 0
        out = np.zeros((count, 96), dtype=np.uint32)
        self._ck(self.L.sipp_inner_products(self.h, g1.ctypes.data, g2.ctypes.data, g1.shape[0] // count, count,
                                            out.ctypes.data), "inner_products")
        return out

    def prove_native(self, A, B):
        """sipp_prove_native: A [n, 16], B [n, 32] uint32 limbs -> proof [2 log2 n + 1, 96]"""
        A = np.ascontiguousarray(A, dtype=np.uint32).reshape(-1, 16)
        B = np.ascontiguousarray(B, dtype=np.uint32).reshape(-1, 32)
        n = A.shape[0]
        words = self.L.sipp_native_proof_words(n)
        if words == 0 or B.shape[0] != n:
            raise SippError(-1, "prove_native: n must be a power of two")
        proof = np.zeros((words // 96, 96), dtype=np.uint32)
        self._ck(self.L.sipp_prove_native(self.h, A.ctypes.data, B.ctypes.data, n, proof.ctypes.data), "prove_native")
        return proof

    def verify_native(self, A, B, proof):
        """sipp_verify_native -> (accepted, statement, [g1_ios, g2_ios, fq12_ios])"""
        A = np.ascontiguousarray(A, dtype=np.uint32).reshape(-1, 16)
        B = np.ascontiguousarray(B, dtype=np.uint32).reshape(-1, 32)
        proof = np.ascontiguousarray(proof, dtype=np.uint32)
        n = A.shape[0]
        lg = n.bit_length() - 1
        st = np.zeros(48 * n + 240, dtype=np.uint32)
        ios = [np.zeros((max(n - 1, 0), 56), dtype=np.uint32), np.zeros((max(n - 1, 0), 104), dtype=np.uint32),
               np.zeros((2 * lg, 296), dtype=np.uint32)]
        ok = C.c_int(0)
        self._ck(self.L.sipp_verify_native(self.h, A.ctypes.data, B.ctypes.data, n, proof.ctypes.data, st.ctypes.data,
                                           ios[0].ctypes.data, ios[1].ctypes.data, ios[2].ctypes.data, C.byref(ok)),
                 "verify_native")
        return bool(ok.value), st, ios

    def prove_native_ex(self, A, B, lists=True, check=True, statement=True, out=None):
        """sipp_prove_native_ex: prove_native and verify_native in one pass -> (proof, accepted, statement, [g1_ios, g2_ios, fq12_ios]).
        lists=False / statement=False / check=False pass NULL for the three lists / the statement / `accepted` and return None in
        their place (all three off: what prove_native launches and nothing more).  out: optional dict of caller arrays keyed "proof",
        "statement", "g1", "g2", "fq12" (native_output_shapes(n)); an output that is asked for is written into the caller's array,
        one that is not asked for is never handed to the library."""
        A, B, n, _ = native_points(A, B, "prove_native_ex")
        shp = native_output_shapes(n)
        proof = _native_out(out, "proof", shp["proof"], "prove_native_ex")
        st = _native_out(out, "statement", shp["statement"], "prove_native_ex") if statement else None
        ios = [_native_out(out, k, shp[k], "prove_native_ex") for k in ("g1", "g2", "fq12")] if lists else None
        ok = C.c_int(0)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._ck(self.L.sipp_prove_native_ex(self.h, A.ctypes.data, B.ctypes.data, n, proof.ctypes.data, ptr(st),
                                             ptr(ios and ios[0]), ptr(ios and ios[1]), ptr(ios and ios[2]),
                                             C.byref(ok) if check else None), "prove_native_ex")
        return proof, (bool(ok.value) if check else None), st, ios

    def prove_async(self, kind, ios):
        """start one sub-proof on the ctx's worker thread (sipp_prove_async); collect it with wait()"""
        ios = np.ascontiguousarray(ios, dtype=np.uint32)
        cap = self.L.sipp_proof_size(self.h, kind, ios.shape[0])
        if cap == 0:
            raise SippError(-1, "sipp_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        self._ck(self.L.sipp_prove_async(self.h, kind, ios.ctypes.data, ios.shape[0], out.ctypes.data, cap), "prove_async")
        self._inflight = (ios, out)      # both buffers stay alive until wait()
        return self

    def wait(self):
        n = C.c_size_t()
        rc = self.L.sipp_wait(self.h, C.byref(n))
        ios, out = getattr(self, "_inflight", None) or (None, None)
        self._inflight = None
        self._ck(rc, "wait")
        return out[: n.value]

    def poseidon_permute(self, states):
        self._ck(self.L.sipp_poseidon_permute(self.h, states.data_ptr(), states.shape[0]), "poseidon_permute")
        return states

    # ---- measurement ----
    def profile(self, enable=True):
        self._ck(self.L.sipp_profile_enable(self.h, int(enable)), "profile_enable")

    def profile_reset(self):
        self._ck(self.L.sipp_profile_reset(self.h), "profile_reset")

    def profile_report(self):
        buf = C.create_string_buffer(1 << 16)
        self._ck(self.L.sipp_profile_report(self.h, buf, len(buf)), "profile_report")
        return json.loads(buf.value.decode())

    def timer_start(self):
        self._ck(self.L.sipp_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.L.sipp_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value


class Instance:
    """The three sub-proofs of one SIPP instance (reference src/verifier_circuit.rs:133-135) on three ctxs = three HIP
    streams, started together through sipp_instance_prove.  `devices` may name one GPU (default) or three
    (level L-B).  `priorities`: stream level per kind ("high" = a high-priority stream; "low" / "" = a stream with a hardware queue of its own at
    normal priority, see sipp_ctx_set_stream_priority in include/sipp_hip.h); G1 low / G2 normal / Fq12 high
    measured best with the start gate of sipp_instance_prove (69.3 vs 71.2 ms per n = 128 instance for low / high / high)."""

    # three concurrent arenas above this share of the card's memory -> one ctx, the proofs back to back (sipp_instance_prove with
    # three equal handles): of the BASELINE configs only the HARDENED n = 4096 instance on ONE GPU (276 GB of 288 GB; the plain one's
    # 246 GB fit).  Measured (scripts/large_n_modes.py, round 4): back to back costs 5.5 % at n = 4096 (1234 against 1169 ms, plain) and
    # 13 - 15 % at n = 1024 (357 against 311 ms) -- so three streams wherever they fit.
    SINGLE_CTX_SHARE = 0.9

    def __init__(self, num_io, devices=(0, 0, 0), priorities=None, hardened=False, single_ctx=None):
        """hardened: G1 / G2 with the hardened AIRs (kinds 4 / 5 in the proofs' headers; sipp_ctx_set_hardened).
        single_ctx: True = one ctx / one arena, the three proofs back to back; False = three ctxs on three streams; None = three
        unless their arenas together exceed SINGLE_CTX_SHARE of the device's memory (and the devices are one device).
        priorities=None: ("low", "", "high") for both AIR variants.  (Until the thin trees' hasher moved to the matrix pipe in round 4 a
        hardened instance wanted G2 on a high-priority stream too: 64.0 - 64.2 against 66.9 - 68.1 ms.  With the shorter Fq12 chain the
        settings are level -- scripts/sweep_prios.sh, two passes: single 56.4 - 57.5 for both, five queued 49.7 - 49.9 against 50.9 ms.)"""
        if priorities is None:
            priorities = ("low", "", "high")
        self.L = lib()
        self.num_io = tuple(int(x) for x in num_io)
        self.ctxs = []
        level = {"low": -1, "": 0, "normal": 0, "high": 1}
        ws = [self.L.sipp_workspace_bytes(k + 4 if (hardened and k < 2) else k, max(1, self.num_io[k])) for k in range(3)]
        if single_ctx is None:
            # three arenas only where they fit what is FREE on the card now (other instances, a queue's earlier slots, torch's pool)
            single_ctx = len(set(devices)) == 1 and sum(ws) > min(self.SINGLE_CTX_SHARE * device_memory_bytes(devices[0]),
                                                                  device_free_bytes(devices[0]))
        self.single_ctx = bool(single_ctx)
        try:
            if self.single_ctx:
                c = Ctx(device=devices[0], workspace_bytes=max(ws))
                self.ctxs = [c, c, c]
                if hardened:
                    c._ck(self.L.sipp_ctx_set_hardened(c.h, 1), "set_hardened")
            else:
                for k in range(3):
                    c = Ctx(device=devices[k], workspace_bytes=ws[k])
                    self.ctxs.append(c)
                    if hardened:
                        c._ck(self.L.sipp_ctx_set_hardened(c.h, 1), "set_hardened")
                    c._ck(self.L.sipp_ctx_set_stream_priority(c.h, level[priorities[k]]), "set_stream_priority")
        except Exception:
            self.close()          # the ctxs (and their arenas) created so far
            raise
        self.caps = [self.L.sipp_proof_size(self.ctxs[k].h, k, self.num_io[k]) if self.num_io[k] else 0 for k in range(3)]
        self.out = [np.zeros(max(c, 1), dtype=np.uint64) for c in self.caps]

    def prove(self, ios):
        """ios: [g1, g2, fq12] host uint32 arrays -> three flat proofs (views of this object's output buffers); a kind with
        no record (an IO shard may have none) yields an empty proof"""
        ios = [np.ascontiguousarray(a, dtype=np.uint32) for a in ios]
        assert tuple(a.shape[0] for a in ios) == self.num_io
        h = (vp * 3)(*[c.h for c in self.ctxs])
        pi = (vp * 3)(*[a.ctypes.data for a in ios])
        ni = (C.c_size_t * 3)(*self.num_io)
        po = (vp * 3)(*[o.ctypes.data for o in self.out])
        pc = (C.c_size_t * 3)(*self.caps)
        pl = (C.c_size_t * 3)()
        rc = self.L.sipp_instance_prove(h, pi, ni, po, pc, pl)
        if rc != 0:
            msgs = "; ".join(self.L.sipp_last_error(c.h).decode() for c in self.ctxs)
            raise SippError(rc, "instance_prove: " + msgs)
        return [self.out[k][: pl[k]] for k in range(3)]

    def flow(self, native_ctx, A, B):
        """sipp_flow_prove: the points A [n, 16], B [n, 32] -> (three flat proofs, native proof, statement, accepted).  native_ctx:
        the Ctx of the native chain (it may be one of this object's); this object's num_io must be (n - 1, n - 1, 2 log2 n)."""
        A, B, n, lg = native_points(A, B, "flow")
        if self.num_io != (n - 1, n - 1, 2 * lg):
            raise SippError(-1, "flow: this Instance was sized for num_io = %r, n = %d needs %r" % (self.num_io, n, (n - 1, n - 1, 2 * lg)))
        shp = native_output_shapes(n)
        nproof, st = np.zeros(shp["proof"], dtype=np.uint32), np.zeros(shp["statement"], dtype=np.uint32)
        h = (vp * 3)(*[c.h for c in self.ctxs])
        po = (vp * 3)(*[o.ctypes.data for o in self.out])
        pc = (C.c_size_t * 3)(*self.caps)
        pl = (C.c_size_t * 3)()
        ok = C.c_int(0)
        rc = self.L.sipp_flow_prove(native_ctx.h, h, A.ctypes.data, B.ctypes.data, n, nproof.ctypes.data, st.ctypes.data, po, pc, pl,
                                    C.byref(ok))
        if rc != 0:
            msgs = "; ".join(self.L.sipp_last_error(c.h).decode() for c in [native_ctx] + self.distinct_ctxs())
            raise SippError(rc, "flow_prove: " + msgs)
        return [self.out[k][: pl[k]] for k in range(3)], nproof, st, bool(ok.value)

    def distinct_ctxs(self):
        return self.ctxs[:1] if getattr(self, "single_ctx", False) else list(self.ctxs)

    def sync(self):
        for c in self.distinct_ctxs():
            c.sync()

    def close(self):
        for c in self.distinct_ctxs():
            c.close()
        self.ctxs = []


class InstanceQueue:
    """sipp_instances_prove: `in_flight` slots of three ctxs on one device; prove(list of [g1, g2, fq12]) proves every instance of
    the list, `in_flight` at a time, and returns their proofs (copies)."""

    def __init__(self, num_io, in_flight=3, device=0, priorities=None, hardened=False):
        """priorities=None: Instance's own default"""
        self.L = lib()
        self.num_io = tuple(int(x) for x in num_io)
        self.slots = []
        # every slot needs three DISTINCT ctxs (sipp_instances_prove refuses duplicate handles): no one-ctx fallback here -- say so
        # before the first hipMalloc instead of failing in the middle of the slots
        need = in_flight * sum(self.L.sipp_workspace_bytes(k + 4 if (hardened and k < 2) else k, max(1, self.num_io[k])) for k in range(3))
        free = device_free_bytes(device)
        if need > free:
            raise SippError(-3, "InstanceQueue: %d slots x three arenas need %.1f GB, %.1f GB are free on device %d; lower in_flight "
                                "(or prove such instances one at a time through Instance, which falls back to one arena)"
                            % (in_flight, need / 2**30, free / 2**30, device))
        try:
            for _ in range(in_flight):
                self.slots.append(Instance(self.num_io, devices=(device,) * 3, priorities=priorities, hardened=hardened, single_ctx=False))
        except Exception:
            self.close()
            raise

    def prove(self, instances):
        count, F = len(instances), len(self.slots)
        keep = [[np.ascontiguousarray(a, dtype=np.uint32) for a in inst] for inst in instances]
        for inst in keep:
            assert tuple(a.shape[0] for a in inst) == self.num_io
        caps = self.slots[0].caps
        outs = [[np.zeros(max(c, 1), dtype=np.uint64) for c in caps] for _ in range(count)]
        h = (vp * (3 * F))(*[c.h for s in self.slots for c in s.ctxs])
        pi = (vp * (3 * count))(*[a.ctypes.data for inst in keep for a in inst])
        ni = (C.c_size_t * (3 * count))(*[n for _ in range(count) for n in self.num_io])
        po = (vp * (3 * count))(*[o.ctypes.data for inst in outs for o in inst])
        pc = (C.c_size_t * (3 * count))(*[c for _ in range(count) for c in caps])
        pl = (C.c_size_t * (3 * count))()
        st = (C.c_int * count)()
        rc = self.L.sipp_instances_prove(h, F, count, pi, ni, po, pc, pl, st)
        if rc != 0:
            msgs = "; ".join(self.L.sipp_last_error(c.h).decode() for s in self.slots for c in s.ctxs)
            raise SippError(rc, "instances_prove: " + msgs)
        return [[outs[i][k][: pl[3 * i + k]] for k in range(3)] for i in range(count)]

    def flows(self, native_ctx, instances, raise_on_error=True):
        """sipp_flows_prove: instances = list of (A [n, 16], B [n, 32]), all of one n with (n - 1, n - 1, 2 log2 n) = this queue's num_io.
        The native chain of every instance runs on native_ctx (a Ctx that is none of the slots') beside the proofs of the instances
        before it.  Returns a list of (three flat proofs, native proof, statement, accepted), copies.  raise_on_error=False returns
        (rc, status list, that list) instead of raising; an instance that failed has empty proofs."""
        count, F = len(instances), len(self.slots)
        n = None
        keep = []
        for A, B in instances:
            A, B, ni, lg = native_points(A, B, "flows")
            if n is None:
                n = ni
            if ni != n or self.num_io != (ni - 1, ni - 1, 2 * lg):
                raise SippError(-1, "flows: every instance must have the n this queue was sized for (num_io = %r)" % (self.num_io,))
            keep.append((A, B))
        if n is None:                              # an empty queue: n follows from num_io
            n = self.num_io[0] + 1
        shp = native_output_shapes(n)
        caps = self.slots[0].caps
        outs = [[np.zeros(max(c, 1), dtype=np.uint64) for c in caps] for _ in range(count)]
        nproofs = [np.zeros(shp["proof"], dtype=np.uint32) for _ in range(count)]
        sts = [np.zeros(shp["statement"], dtype=np.uint32) for _ in range(count)]
        h = (vp * (3 * F))(*[c.h for s in self.slots for c in s.ctxs])
        pa = (vp * count)(*[a.ctypes.data for a, _ in keep])
        pb = (vp * count)(*[b.ctypes.data for _, b in keep])
        pn = (vp * count)(*[a.ctypes.data for a in nproofs])
        ps = (vp * count)(*[a.ctypes.data for a in sts])
        po = (vp * (3 * count))(*[o.ctypes.data for inst in outs for o in inst])
        pc = (C.c_size_t * (3 * count))(*[c for _ in range(count) for c in caps])
        pl = (C.c_size_t * (3 * count))()
        acc = (C.c_int * count)()
        st = (C.c_int * count)()
        rc = self.L.sipp_flows_prove(native_ctx.h, h, F, count, n, pa, pb, pn, ps, po, pc, pl, acc, st)
        res = [([outs[i][k][: pl[3 * i + k]] for k in range(3)], nproofs[i], sts[i], bool(acc[i])) for i in range(count)]
        if not raise_on_error:
            return rc, list(st), res
        if rc != 0:
            msgs = "; ".join(self.L.sipp_last_error(c.h).decode() for c in [native_ctx] + [c for s in self.slots for c in s.ctxs])
            raise SippError(rc, "flows_prove: " + msgs)
        return res

    def close(self):
        for s in self.slots:
            s.close()
        self.slots = []



class CircuitData:
    """plonky2's CircuitData for the outer proof over HOST arrays (sipp_circuit_build / _prove / _verify: reference
    src/verifier_circuit.rs:225, :253, :254): the gate set, the generators with their level schedule and the constants_sigmas values go in
    once; prove() takes the wire table with its input cells set and the public inputs, both numpy, and returns the flat proof."""

    def __init__(self, ctx, log_n, params, fri, circuit, constants_sigmas, gens, sched=None, digest=None, hasher=None):
        """hasher: None = sipp_circuit_build; 'poseidon' / 'keccak' = sipp_circuit_build_h (the data's commitment, proofs and verify follow it)"""
        self.ctx, self.L = ctx, ctx.L                      # the ctx must outlive this object
        self.circuit, self.params, self.fri = circuit, params, fri
        cs = np.ascontiguousarray(constants_sigmas, dtype=np.uint64)
        arr = _gen_array(gens)
        self._sched = None if sched is None else PlonkScheduleHost.from_dict(sched)
        h = C.c_void_p()
        head = [ctx.h, log_n, C.byref(params), C.byref(fri), C.byref(circuit), cs.ctypes.data, arr, len(gens),
                None if self._sched is None else C.byref(self._sched), None if digest is None else ctx._u64([int(x) for x in digest])]
        if hasher is None:
            rc = self.L.sipp_circuit_build(*head, C.byref(h))
        else:
            rc = self.L.sipp_circuit_build_h(*head, hasher_id(hasher), C.byref(h))
        ctx._ck(rc, "circuit_build")
        self.h, self.num_wires, self.n = h, circuit.num_wires, 1 << log_n
        cap = np.zeros(((1 << min(fri.cap_height, log_n + fri.rate_bits)), 4), dtype=np.uint64)
        dg = np.zeros(4, dtype=np.uint64)
        ctx._ck(self.L.sipp_circuit_verifier_data(self.h, cap.ctypes.data, dg.ctypes.data), "circuit_verifier_data")
        self.cap, self.digest = cap, dg
        self.input_map = None                              # (n_words, n_extra) once set_input_map has been served
        self.lookup = None                                 # the eight words once set_lookup has been served

    def prove(self, wires, public_inputs):
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        if w.shape != (self.num_wires, self.n):
            raise SippError(-1, "CircuitData.prove: wires must be [num_wires][N]")
        pis = [int(x) for x in public_inputs]
        cap = self.L.sipp_circuit_proof_size(self.h, len(pis))
        if cap == 0:
            raise SippError(-1, "sipp_circuit_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        self.ctx._ck(self.L.sipp_circuit_prove(self.h, w.ctypes.data, self.ctx._u64(pis) if pis else None, len(pis), out.ctypes.data, cap, C.byref(n)),
                     "circuit_prove")
        return out[: n.value]

    def prove_inputs(self, cells, values, public_inputs):
        """prove() from the input cells alone (sipp_circuit_prove_inputs): cells[k] = wire * N + row takes values[k], every other cell
        starts 0; the proof is prove()'s for that table"""
        cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        if len(cells) != len(values):
            raise SippError(-1, "CircuitData.prove_inputs: cells and values differ in length")
        pis = [int(x) for x in public_inputs]
        cap = self.L.sipp_circuit_proof_size(self.h, len(pis))
        if cap == 0:
            raise SippError(-1, "sipp_circuit_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        self.ctx._ck(self.L.sipp_circuit_prove_inputs(self.h, cells.ctypes.data if len(cells) else None, values.ctypes.data if len(cells) else None,
                                                      len(cells), self.ctx._u64(pis) if pis else None, len(pis), out.ctypes.data, cap, C.byref(n)),
                     "circuit_prove_inputs")
        return out[: n.value]

    def set_input_map(self, cells, sources, n_words, n_extra):
        """sipp_circuit_set_input_map: cells[k] takes word sources[k] of words || extra (n_words, n_extra u64) in every later
        prove_words; a second call replaces the map, a refused one leaves it"""
        cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
        sources = np.ascontiguousarray(sources, dtype=np.uint64).reshape(-1)
        if len(cells) != len(sources):
            raise SippError(-1, "CircuitData.set_input_map: cells and sources differ in length")
        self.ctx._ck(self.L.sipp_circuit_set_input_map(self.h, cells.ctypes.data if len(cells) else None, sources.ctypes.data if len(cells) else None,
                                                       len(cells), int(n_words), int(n_extra)), "circuit_set_input_map")
        self.input_map = (int(n_words), int(n_extra))

    def prove_words(self, words, extra, public_inputs):
        """prove_inputs() with the values gathered on the device (sipp_circuit_prove_words): the map of set_input_map says which cell
        takes which word of words || extra"""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        extra = np.ascontiguousarray(extra, dtype=np.uint64).reshape(-1)
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1)
        cap = self.L.sipp_circuit_proof_size(self.h, len(pis))
        if cap == 0:
            raise SippError(-1, "sipp_circuit_proof_size")
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        self.ctx._ck(self.L.sipp_circuit_prove_words(self.h, words.ctypes.data if len(words) else None, len(words),
                                                     extra.ctypes.data if len(extra) else None, len(extra),
                                                     pis.ctypes.data_as(C.POINTER(C.c_uint64)) if len(pis) else None, len(pis), out.ctypes.data, cap,
                                                     C.byref(n)), "circuit_prove_words")
        return out[: n.value]

    def set_blinding(self, seed):
        """sipp_circuit_set_blinding: the seed (four canonical words) of a circuit data built with fri.hiding = 1; the counter restarts
        at 0 and every prove call uses the next number"""
        self.ctx._ck(self.L.sipp_circuit_set_blinding(self.h, self.ctx._u64(seed)), "circuit_set_blinding")

    def set_lookup(self, lookup):
        """sipp_circuit_set_lookup: the eight-word lookup description; every later prove call runs the multiplicities behind witness
        generation and proves the lookup argument ("SIPPPLK4"), verify() checks it.  An empty description takes it off again."""
        self.ctx._ck(self.L.sipp_circuit_set_lookup(self.h, Ctx._lookup_words(lookup)), "circuit_set_lookup")
        self.lookup = tuple(int(x) for x in lookup)

    def verify(self, proof):
        """-> (status, refusing stage): (0, 0) = accepted"""
        pf = np.ascontiguousarray(proof, dtype=np.uint64)
        reason = C.c_int(0)
        rc = self.L.sipp_circuit_verify(self.h, pf.ctypes.data, len(pf), C.byref(reason))
        return rc, reason.value

    def close(self):
        if self.h:
            self.L.sipp_circuit_destroy(self.h)
            self.h = None


def io_shard(num_io, world, rank):
    """sipp_io_shard: the contiguous range (first, count) of an obligation list that `rank` of `world` proves"""
    first, count = C.c_size_t(), C.c_size_t()
    rc = lib().sipp_io_shard(int(num_io), int(world), int(rank), C.byref(first), C.byref(count))
    if rc != 0:
        raise SippError(rc, "io_shard")
    return first.value, count.value


def shard_ios(ios, world, rank):
    """IO-sharded sub-proofs (level L-D): the slices of the three obligation lists of ONE SIPP instance
    that `rank` proves as STARKs of their own; no data is exchanged between the ranks"""
    out = []
    for a in ios:
        first, count = io_shard(a.shape[0], world, rank)
        out.append(a[first: first + count])
    return out
