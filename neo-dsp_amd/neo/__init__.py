"""neo (MI355X): the FFT + UPOLS hot path of neo-dsp on HIP/gfx950.

`import neo` mirrors the reference's Python package entry points that exist on
this path (extra/python/src/neo/__init__.py, neo/fft/__init__.py); the compute
is libneo_hip.so (include/neo_hip.h). Put `<repo>/neo-dsp_amd` on sys.path.
"""
from . import _native
from . import convolution
from . import fft
from .convolution import (UpolsConvolver, UpolsConvolver64, upols64_plan, upols64_batch_plan, upols64_offline_plan, UpolsMultiConvolver, convolve, dense_convolve, direct_convolve, fft_convolve,
                          host_register, host_unregister, memory_info, memory_trim, normalize_impulse, overlap_add, overlap_save, OverlapStage, UpolsGroup,
                          num_partitions, split_upola_convolver, split_upols_convolver, uniform_partition,
                          upola_convolver, upola_convolver_v2, upols_convolver,
                          SparseUpolsConvolver, sparse_convolve, sparse_fade_plan, sparse_plan, sparse_window_plan,
                          sparse_upola_convolver,
                          sparse_upols_convolver, PerceptualSparsity, a_weighting, amplitude_to_db, perceptual_histogram,
                          perceptual_histogram_host, perceptual_mask, perceptual_mask_host, perceptual_weights,
                          threshold_for_tile_density, tile_density_curve,
                          MatrixConvolver, fade_gains, matrix_batch_plan, matrix_convolve, matrix_fade_gains, matrix_level_plan,
                          matrix_offline_plan, matrix_plan)

__version__ = "0.1.0"

__all__ = [
    "fft",
    "convolution",
    "UpolsConvolver",
    "UpolsConvolver64",
    "upols64_plan",
    "upols64_batch_plan",
    "upols64_offline_plan",
    "UpolsMultiConvolver",
    "upols_convolver",
    "split_upols_convolver",
    "upola_convolver",
    "split_upola_convolver",
    "upola_convolver_v2",
    "uniform_partition",
    "normalize_impulse",
    "num_partitions",
    "overlap_save",
    "overlap_add",
    "OverlapStage",
    "UpolsGroup",
    "host_register",
    "host_unregister",
    "memory_info",
    "memory_trim",
    "dense_convolve",
    "SparseUpolsConvolver",
    "sparse_upols_convolver",
    "sparse_upola_convolver",
    "sparse_plan",
    "sparse_window_plan",
    "sparse_fade_plan",
    "sparse_convolve",
    "MatrixConvolver",
    "matrix_plan",
    "matrix_batch_plan",
    "matrix_offline_plan",
    "matrix_level_plan",
    "matrix_convolve",
    "matrix_fade_gains",
    "fade_gains",
    "a_weighting",
    "amplitude_to_db",
    "PerceptualSparsity",
    "perceptual_weights",
    "perceptual_mask",
    "perceptual_mask_host",
    "perceptual_histogram",
    "perceptual_histogram_host",
    "tile_density_curve",
    "threshold_for_tile_density",
    "convolve",
    "fft_convolve",
    "direct_convolve",
]
