"""aircombat-selfplay_amd — MI355X-native vectorised air-combat ``step()``.

Host-side mirror of the reference's VecEnv surface (``envs/env_wrappers.py``) over the C ABI of
``include/aircombat.h`` (``libaircombat_hip.so``: hand-written HIP kernels for gfx950).

The directory name carries a hyphen, so import it as ``importlib.import_module("aircombat-selfplay_amd")``
or through the repo-root alias module ``aircombat_selfplay_amd``.
"""
from .capi import AcConfig, AcInitState, Lib, load_library, library_path, HipExtensionMissing  # noqa: F401
from .config import config_from_yaml, default_config, default_nvn_config, curriculum_bank, TASK_IDS  # noqa: F401
from .vec_env import HipVecEnv, HipShareVecEnv, MultiDeviceVecEnv, make_env, controller_forward  # noqa: F401
from .rollout_buffer import DeviceReplayBuffer, DeviceSharedReplayBuffer, DeviceEpoch  # noqa: F401
from .snapshot import EnvSnapshot, MultiSnapshot, SnapshotMismatch  # noqa: F401
from .policy import DevicePolicy, DeviceMAPPOPolicy, DevicePolicyPool, UnsupportedPolicy  # noqa: F401
from .rollout import DeviceRollout, DeviceMAPPORollout  # noqa: F401
from .evaluate import DeviceEvaluator, EvalResult, elo_update  # noqa: F401
from .league import DeviceLeague, LeagueTable, round_robin  # noqa: F401
from .recorder import FlightRecorder  # noqa: F401
from .spawn import SpawnCurriculum  # noqa: F401
from . import sharding  # noqa: F401

_TORCH_EXPORTS = {"DeviceGRUFunction": "gru_train", "DeviceGRULayer": "gru_train", "use_device_gru": "gru_train",
                  "DeviceGRULayerFunction": "gru_layer_train", "gru_layer": "gru_layer_train", "DeviceFusedGRULayer": "gru_layer_train",
                  "use_device_gru_layer": "gru_layer_train",
                  "DeviceMLPBlockFunction": "mlp_train", "DeviceMLPLayer": "mlp_train", "mlp_block": "mlp_train", "use_device_mlp": "mlp_train",
                  "DeviceActEvalFunction": "act_train", "act_evaluate": "act_train", "use_device_act": "act_train",
                  "DevicePPOLossFunction": "ppo_update", "ppo_loss": "ppo_update", "device_clip_adam_step": "ppo_update", "DevicePPOTrainer": "ppo_update",
                  "DeviceDiscriminator": "mutual_support",
                  "DeviceActorEvalFunction": "net_train", "DeviceCriticFunction": "net_train", "value_head": "net_train", "feature_norm": "net_train",
                  "shoot_prior": "net_train", "use_device_networks": "net_train"}


def __getattr__(name):
    # the training layers' classes derive from torch's: loaded on first use, so importing the package does not import torch
    if name in _TORCH_EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _TORCH_EXPORTS[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

__all__ = ["AcConfig", "AcInitState", "Lib", "load_library", "library_path", "HipExtensionMissing",
           "config_from_yaml", "default_config", "default_nvn_config", "TASK_IDS", "HipVecEnv", "HipShareVecEnv", "MultiDeviceVecEnv", "make_env", "controller_forward",
           "DeviceReplayBuffer", "DeviceSharedReplayBuffer", "DeviceEpoch", "EnvSnapshot", "MultiSnapshot", "SnapshotMismatch",
           "DevicePolicy", "DeviceMAPPOPolicy", "DevicePolicyPool", "UnsupportedPolicy", "DeviceRollout", "DeviceMAPPORollout", "DeviceEvaluator", "EvalResult", "elo_update", "DeviceLeague", "LeagueTable", "round_robin", "FlightRecorder", "SpawnCurriculum", "curriculum_bank", "DeviceGRUFunction", "DeviceGRULayer", "use_device_gru",
           "DeviceGRULayerFunction", "gru_layer", "DeviceFusedGRULayer", "use_device_gru_layer",
           "DeviceMLPBlockFunction", "DeviceMLPLayer", "mlp_block", "use_device_mlp",
           "DeviceActEvalFunction", "act_evaluate", "use_device_act",
           "DevicePPOLossFunction", "ppo_loss", "device_clip_adam_step", "DevicePPOTrainer", "DeviceDiscriminator",
           "DeviceActorEvalFunction", "DeviceCriticFunction", "value_head", "feature_norm", "shoot_prior", "use_device_networks"]
