"""MI355X-native Monte-Carlo relative-Viterbi-metric detector.

Drop-in for the hot path of So-bonkers/Detecting-Convolutional-Codes-Via-Markovian-Statistics
(Pd_plotter.run_experiment and the functions beneath it), running on gfx950
through libcvd.so (include/cvd.h).  See DESIGN.md.
"""
from ._lib import CvdError, lib, PATH_AUTO, PATH_TABLE, PATH_EXPLICIT, PATH_EXPLICIT_GENERIC, PATH_EXPLICIT_ORBIT, PATH_EXPLICIT_BUTTERFLY, KERNEL_NAMES, CAPTURE_LSB, CAPTURE_MSB, CAPTURE_BYTES  # noqa: F401
from .codes import Code, EXAMPLE_CODES, CONFIG_CODES, octal_to_taps  # noqa: F401
from .detector import (  # noqa: F401
    DEFAULTS, N_SPECTRUM_BY_M, Detector, Model, run_experiment, learn_P1_empirical,
    enumerate_markov_states_allzero, build_trellis, branch_output_and_next_state,
    viterbi_metric_step, simulate_markov_sequence, log_likelihood_ratio, grid_tag, LEARN_TAG,
    enumerate_states_device, scan_capture, capture_buffer,
)
from .parity import (  # noqa: F401
    parse_poly_token, build_parity_system, nullspace_mod2, parity_vector_to_equation, parity_vectors,
    template_of, default_template, parity_detect, parity_satisfaction_fraction, parity_detector,
    parity_experiment, encode_convolutional,
)
from .encode import encode_capture, encode_frames, pack_info, unpack_info  # noqa: F401
from .blind import (  # noqa: F401
    template_mask, mask_template, mask_extent, parity_sweep, find_parity_checks, identify_code, default_z_min,
)
from .decode import (PUNCTURE_PATTERNS, decode_capture, decode_capture_punctured, decode_capture_soft,  # noqa: F401
                     decode_frames, decode_frames_llr, decode_frames_llr_punctured, decode_frames_soft,
                     decode_frames_soft_punctured, decode_frames_tailbiting, decode_frames_tailbiting_soft,
                     decode_frames_tailbiting_soft_punctured, depuncture_soft, puncture_pattern, punctured_bits,
                     soft_from_bits, sync_punctured, sync_punctured_soft,
                     CRC_SPECS, crc_spec, decode_frames_crc, decode_frames_list, frames_crc,
                     decode_frames_tailbiting_crc, decode_frames_tailbiting_list)
from .exponent import (  # noqa: F401
    TransitionTensor, learn_transition_tensor, chernoff_rhos, compute_error_exponent, spectral_radius,
    fit_error_exponent, EXPONENT_TAG,
)
