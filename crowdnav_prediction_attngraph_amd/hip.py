"""The import surface of the boundary calls: thin object wrappers over the C ABI handles and the rollout / training entry points.  Their homes
are hip_env (simulator, rendering, stamps), hip_policy (the policy handles), hip_train (the training path) and gst_hip (the GST predictor)."""
import ctypes as C  # noqa: F401
import math  # noqa: F401

import torch  # noqa: F401

from . import _abi as A  # noqa: F401
from .gst_hip import HipGST  # noqa: F401
from .hip_env import (HipEnvBatch, StepStamps, orca_solve, prediction_dots, render_scenes, render_trajectories, tile_images,  # noqa: F401
                      trace_metrics)
from .hip_policy import HipHandle, HipPolicy, HipSrnn, compact_visible  # noqa: F401
from .hip_train import (Embed0, GRUSequence, HHAttention, HHBlockFused, HipLinear, HRAttention, MinibatchStepper, PPOLoss, RightMatmul,  # noqa: F401
                        RnSequence, SizedMinibatchStepper, SmallMM, SrnnAttention, SrnnEdgeSequence, WgradLinear, adam_clip_step, adv_normalize, adv_stats, gae, linear_act,
                        linear_supported, split_bf16, weight_mm, wgrad, wgrad_supported)
