"""The bounds the per-node gradient parity tests assert, in one place: the tests that established them and the autograd
contract sweep (tests/test_gpu_autograd_contract.py) read the same numbers.  Each entry names the test that owns it."""

# test_gpu_backbone.py::test_conv_bn_act_function_matches_the_autocast_chain — relative L2 error of the fused node against the
# high-precision chain: no larger than 1.5 x the bf16 autocast chain's own error (floor 1e-2), and below 8e-2 whatever the chain does
CONV_BN_ACT_CHAIN_FACTOR = 1.5
CONV_BN_ACT_FLOOR = 1e-2
CONV_BN_ACT_CAP = 8e-2


def conv_bn_act_within_bound(err_fused, err_chain):
    return err_fused <= max(CONV_BN_ACT_CHAIN_FACTOR * err_chain, CONV_BN_ACT_FLOOR) and err_fused < CONV_BN_ACT_CAP


# test_gpu_backbone.py::test_training_backbone_fused_nodes_match_the_autocast_modules — max-norm relative differences
BACKBONE_FUSED_OUT_REL = 0.06
BACKBONE_FUSED_GRAD_MEDIAN_REL = 0.05
BACKBONE_FUSED_GRAD_WORST_REL = 0.5

# test_gpu_backward.py::test_autograd_function_round_trip — max|got - ref| / max(1, max|ref|)
MSDA_GRAD_TOL = 1e-4

# test_gpu_sca_fused_backward.py::test_op_matches_float64_restatement — max|got - ref| <= REL * max|ref| + ABS
SCA_FUSED_GRAD_REL = 1e-4
SCA_FUSED_GRAD_ABS = 1e-6

# test_gpu_decoder.py::test_conv3d_autograd_function_matches_float64_autograd — max abs differences (dW: x max(1, max|dW|))
CONV3D_OUT_ABS = 1e-4
CONV3D_DX_ABS = 2e-4
CONV3D_DW_ABS = 2e-4

# test_gpu_linear.py::test_linear_autograd_function_matches_f64_autograd — max|got - ref| / max|ref|, output and gradients
LINEAR_X3_REL = 2e-4

# test_gpu_linear.py::test_linear_wgrad_matches_f64 — max|got - ref| / max|ref|
LINEAR_WGRAD_DW_REL = 1e-4
LINEAR_WGRAD_DB_REL = 1e-3

# test_gpu_training.py::test_rows_gather_sum_matches_torch_index_ops_and_gradient — the output is a copy, the gradient max abs
ROWS_GATHER_OUT_ABS = 0.0
ROWS_GATHER_GRAD_ABS = 1e-5

# test_gpu_training.py::test_sca_prep_function_matches_torch_ops_and_gradient — max abs (loc, attn), max-norm relative (gradient)
SCA_PREP_LOC_ABS = 1e-5
SCA_PREP_ATTN_ABS = 1e-6
SCA_PREP_GRAD_REL = 1e-5

# test_gpu_training.py::test_dropout_add_layernorm_node_matches_torch — max|got - ref| / (max|ref| + 1e-12)
DROPOUT_LN_REL = 2e-5
