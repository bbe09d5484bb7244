"""co-snarks_amd -- MI355X (gfx950) proof-generation hot path for TaceoLabs/co-snarks.

The product is two native libraries built in-tree by ``build.py``:

* ``lib/libcosnarks_hip.so``      -- the C ABI declared in ``include/cosnarks_hip.h`` (hand-written HIP:
  Pippenger MSM, LDS-tiled radix-2 NTT, Rep3/Shamir share-vector arithmetic);
* ``lib/libcosnarks_groth16.so``  -- C++ host mirror of the reference's ``CircomGroth16Prover`` /
  ``R1CSToQAP`` / ``CoGroth16::prove`` interface, calling only that C ABI.

This Python package is a thin ctypes harness over them (tests, bench, smoke).  There is NO CPU fallback:
every compute call raises ``CoSnarksHipError`` if the library is missing or no HIP device is present.
The directory name contains a hyphen; import it as ``import cosnarks_amd`` (alias module at the repo root)
or ``importlib.import_module("co-snarks_amd")``.
"""
from . import bindings  # noqa: F401
from .bindings import (  # noqa: F401
    BLS12_381,
    BN254,
    GRUMPKIN,
    G1,
    G2,
    Bases,
    CoSnarksHipError,
    Comm,
    DeviceBuffer,
    Domain,
    device_count,
    eval_poly,
    poly_div_linear,
    poly_lincomb,
    fr_bytes,
    groth16_h,
    have_device,
    HonkCoBatch,
    HonkMemoryRecords,
    honk_co_arith,
    honk_co_delta_finish,
    honk_co_delta_operands,
    honk_co_delta_sub_one,
    honk_co_lookup_finish,
    honk_co_lookup_mid,
    honk_co_lookup_operands,
    honk_co_perm_finish,
    honk_co_perm_operands,
    honk_co_perm_operands2,
    honk_co_select_edges,
    honk_lookup_operands,
    honk_perm_operands,
    honk_pow_table,
    honk_sumcheck_accumulate,
    honk_sumcheck_accumulate_gates,
    honk_w4_records,
    honk_z_perm_place,
    lib,
    lib_path,
    lincomb,
    mle_fold,
    mle_fold_rounds,
    msm_fold_partials,
    msm_partial_bytes,
    msm_split,
    plonk_blind_coefficients,
    plonk_quot_blinders,
    plonk_quot_combine,
    plonk_quot_finish,
    plonk_quot_operands,
    plonk_z_operands,
    point_bytes,
    rep3_local_mul_vec,
    rep3_to_shamir_vec,
    tune_get,
    msm_plan,
    tune_set,
    tuned,
    vec_add,
    vec_batch_inverse,
    vec_mul,
    vec_mul_table,
    vec_prefix_prod,
    vec_rotate_right,
    vec_sub,
)
