from bflc_amd.ops import functional
from bflc_amd.ops.functional import (accuracy, accuracy_t, adam_step_,
                                     axpy_, batchnorm2d, conv2d, conv2d_bn,
                                     conv2d_relu_pool,
                                     conv_relu_pool_stack,
                                     global_avgpool, add_relu,
                                     hip_available, hip_ops, linear,
                                     maxpool2d, relu, sgd_step_,
                                     sgdm_step_, grad_clip_coef_,
                                     softmax_cross_entropy, weighted_fedavg,
                                     order_stat_mean, delta_gram,
                                     masked_wmean, grad_clip_final_,
                                     delta_extract_sumsq_, dp_privatize_,
                                     dp_philox_words)

__all__ = [
    "functional", "linear", "conv2d", "conv2d_bn", "conv2d_relu_pool",
    "conv_relu_pool_stack", "batchnorm2d", "relu",
    "add_relu", "maxpool2d", "global_avgpool", "softmax_cross_entropy",
    "accuracy", "accuracy_t", "axpy_", "sgd_step_", "adam_step_",
    "sgdm_step_", "grad_clip_coef_",
    "weighted_fedavg", "order_stat_mean", "delta_gram", "masked_wmean",
    "grad_clip_final_", "delta_extract_sumsq_", "dp_privatize_",
    "dp_philox_words",
    "hip_ops", "hip_available",
]
