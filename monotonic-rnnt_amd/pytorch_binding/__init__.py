"""PyTorch surface of the MI355X monotonic RNN-T loss (drop-in for the reference's pytorch_binding)."""
from .monotonic_rnnt_joint import (MonotonicRNNTJointExpectedCostFunction, MonotonicRNNTJointFunction,
                                   MonotonicRNNTJointHatFunction, MonotonicRNNTJointPathFunction,
                                   monotonic_rnnt_joint_align, monotonic_rnnt_joint_expected_cost,
                                   monotonic_rnnt_joint_hat_loss, monotonic_rnnt_joint_loss,
                                   monotonic_rnnt_joint_path_loss, monotonic_rnnt_joint_posteriors,
                                   monotonic_rnnt_joint_sample)
from .monotonic_rnnt_op import (MonotonicRNNTExpectedCostFunction, MonotonicRNNTFunction, MonotonicRNNTHatFunction,
                                MonotonicRNNTHatLoss, MonotonicRNNTLoss, MonotonicRNNTPathFunction,
                                monotonic_rnnt_align, monotonic_rnnt_cpp, monotonic_rnnt_expected_cost,
                                monotonic_rnnt_hat_loss, monotonic_rnnt_loss, monotonic_rnnt_path_loss,
                                monotonic_rnnt_posteriors, monotonic_rnnt_sample)

__all__ = ["MonotonicRNNTFunction", "monotonic_rnnt_loss", "MonotonicRNNTLoss", "monotonic_rnnt_cpp",
           "MonotonicRNNTJointFunction", "monotonic_rnnt_joint_loss", "monotonic_rnnt_align",
           "monotonic_rnnt_posteriors", "monotonic_rnnt_joint_align", "monotonic_rnnt_joint_posteriors",
           "monotonic_rnnt_sample", "monotonic_rnnt_joint_sample", "MonotonicRNNTPathFunction",
           "monotonic_rnnt_path_loss", "MonotonicRNNTJointPathFunction", "monotonic_rnnt_joint_path_loss",
           "MonotonicRNNTExpectedCostFunction", "monotonic_rnnt_expected_cost",
           "MonotonicRNNTJointExpectedCostFunction", "monotonic_rnnt_joint_expected_cost",
           "MonotonicRNNTHatFunction", "monotonic_rnnt_hat_loss", "MonotonicRNNTHatLoss",
           "MonotonicRNNTJointHatFunction", "monotonic_rnnt_joint_hat_loss"]
