"""MI355X-native BN254 proving hot path (G1/G2 Pippenger MSM + Fr NTT + Groth16 prove) behind the gnark-crypto
call sites that lambdaclass/noir_backend_using_gnark reaches through groth16.Prove / plonk.Prove.

Layout
  csrc/        hand-written HIP kernels for gfx950 + the C ABI (include/zkmi.h) -> libzkmi.so
  _lib.py      ctypes loader (fails loudly when the HIP library or a GPU is missing -- there is no CPU fallback)
  bn254.py     host-side mirror of the gnark-crypto interface for this path (MultiExp, fft.Domain)
  groth16.py   host-side mirror of gnark's groth16 prove for this path (ProvingKey, prove, compute_h)
  plonk.py     host-side mirror of gnark's plonk setup / prove and of iop's copy-constraint ratio for many witnesses (ratio_copy_batch), the quotient's (quotient_batch), the openings' (linearize_batch, open_batch, poly_open_rows) and the digests of their rows (commit_rows), and of the batch prover over them (prove_batch, prove_batch_info, challenges_rows; exported as plonk_*: the Groth16 names are taken)
  parallel.py  one-process-per-GPU sharding of MSMs / proofs with torch.distributed (RCCL)
"""
from . import _lib  # noqa: F401
from .bn254 import (DIF, DIT, Domain, MultiExpConfig, bit_reverse, fr_batch_invert, g1_multi_exp, g2_multi_exp)  # noqa: F401
from .groth16 import R1CS, ProvingKey, compute_h, compute_h_batch, finalize_batch, prove, prove_batch, prove_r1cs, prove_r1cs_batch, setup  # noqa: F401
from .plonk import linearize_batch, open_batch, permutation_sigma, poly_open_rows, quotient_batch, ratio_copy_batch  # noqa: F401
from .plonk import challenges_rows as plonk_challenges_rows, prove_batch as plonk_prove_batch, prove_batch_info as plonk_prove_batch_info  # noqa: F401
from .wire import deserialize_felts, serialize_felts  # noqa: F401

__all__ = ["DIF", "DIT", "Domain", "MultiExpConfig", "bit_reverse", "g1_multi_exp", "g2_multi_exp", "ProvingKey", "compute_h", "prove", "fr_batch_invert",
           "permutation_sigma", "ratio_copy_batch", "quotient_batch", "linearize_batch", "open_batch", "poly_open_rows", "plonk_prove_batch", "plonk_prove_batch_info",
           "plonk_challenges_rows"]
