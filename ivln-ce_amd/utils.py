"""Glue with the reference's names (ivlnce_baselines/common/utils.py:12-135): observation batching
and host->device moves.  No arithmetic."""
from collections import defaultdict
from typing import Dict, List, Optional, Set, Tuple

import numpy as np
import torch


def extract_instruction_tokens(observations: List[Dict], instruction_sensor_uuid: str, tokens_uuid: str = "tokens"):
    """utils.py:12-35."""
    if instruction_sensor_uuid not in observations[0] or instruction_sensor_uuid == "pointgoal_with_gps_compass":
        return observations
    for i in range(len(observations)):
        if isinstance(observations[i][instruction_sensor_uuid], dict) and tokens_uuid in observations[i][instruction_sensor_uuid]:
            observations[i][instruction_sensor_uuid] = observations[i][instruction_sensor_uuid]["tokens"]
        else:
            break
    return observations


def batch_obs(observations: List[Dict], device: Optional[torch.device] = None,
              ignore_keys: Optional[Set[str]] = None) -> Dict:
    """utils.py:57-92: list of per-env dicts -> dict of stacked device tensors (uint32 -> int32;
    `env_name` kept as a list)."""
    if ignore_keys is None:
        ignore_keys = {"env_name"}
    batch = defaultdict(list)
    for obs in observations:
        for sensor in obs:
            v = obs[sensor]
            if isinstance(v, np.ndarray) and v.dtype == np.uint32:
                v = np.int32(v)
            if sensor not in ignore_keys:
                v = torch.as_tensor(v)
            batch[sensor].append(v)
    out: Dict = {}
    for sensor in batch:
        if sensor not in ignore_keys:
            out[sensor] = torch.stack(batch[sensor], dim=0).to(device)
        else:
            out[sensor] = batch[sensor]
    return out


def batch_to(batch: Tuple, device: torch.device = None, non_blocking: bool = True) -> Tuple:
    """utils.py:95-135: observations cast to float32 on the device, the rest moved as is."""
    (observations_batch, prev_actions_batch, episode_not_done_masks, tour_not_done_mask, corrected_actions_batch,
     weights_batch) = batch
    observations_batch = {
        k: v.to(device=device, dtype=torch.float32, non_blocking=non_blocking) for k, v in observations_batch.items()
    }
    return (
        observations_batch,
        prev_actions_batch.to(device=device, non_blocking=non_blocking),
        episode_not_done_masks.to(device=device, non_blocking=non_blocking),
        tour_not_done_mask.to(device=device, non_blocking=non_blocking) if tour_not_done_mask is not None else None,
        corrected_actions_batch.to(device=device, non_blocking=non_blocking),
        weights_batch.to(device=device, non_blocking=non_blocking),
    )


def trim_instruction_padding(observations: Dict, key: str = "instruction", multiple: int = 8,
                             first_rows: Optional[int] = None) -> Dict:
    """Drop the all-padding tail of a HOST-side token batch (rows, 200) before it is copied to the GPU: the
    reference's packed bi-LSTM / pad_packed_sequence only ever produces the batch's longest instruction
    (instruction_encoder.py:70-92), so every consumer (W_ih GEMM, text_k, the attention axis) sees Lmax columns,
    not 200.  Lmax is rounded up to `multiple` (16-byte loads along the token axis); columns beyond a row's own
    length stay masked exactly as before.  A device tensor is returned unchanged (finding Lmax would be a sync).

    `first_rows` = N for a collated time-major (T*N, 200) batch: only the t = 0 rows are measured.  `collate_fn`
    pads the observations of finished trajectories with 1.0 (dagger_trainer.py:66-70), so a padded timestep row
    counts 200 "tokens" and would disable the trim for every batch of unequal trajectory lengths; the instruction
    of a trajectory is the same at every timestep and t = 0 is never padding.  Padded rows keep their first Lmax
    ones - those timesteps carry zero loss weight, so what the encoder makes of them never reaches a gradient."""
    t = observations.get(key)
    if t is None or not torch.is_tensor(t) or t.is_cuda or t.dim() != 2:
        return observations
    L = t.shape[1]
    probe = t if first_rows is None else t[:first_rows]
    longest = int((probe != 0).sum(dim=1).max().item()) if probe.shape[0] > 0 else L
    keep = min(L, max(multiple, -(-longest // multiple) * multiple))
    if keep < L:
        observations = dict(observations)
        observations[key] = t[:, :keep].contiguous()
    return observations


def dedupe_instructions(observations: Dict, key: str = "instruction") -> Dict:
    """HOST side, update batches: a collated time-major batch repeats each trajectory's token row at every timestep
    (T*N rows, N + 1 distinct ones: the trajectories and collate_fn's all-ones padding row).  Adds
    `instruction_unique` (U, L) and `instruction_index` (T*N,) so that the policy encodes U sequences instead of T*N
    (policy.MapCMANet.forward_hip); the gradient is identical - the per-row gradients are summed onto the shared
    encoding in row order.  Left alone when nothing repeats or the tensor is already on the device."""
    t = observations.get(key)
    if t is None or not torch.is_tensor(t) or t.is_cuda or t.dim() != 2 or t.shape[0] < 2:
        return observations
    uniq, inv = torch.unique(t, dim=0, return_inverse=True)
    if uniq.shape[0] * 2 > t.shape[0]:
        return observations
    observations = dict(observations)
    observations[key + "_unique"] = uniq.contiguous()
    observations[key + "_index"] = inv.to(torch.int32).contiguous()
    return observations


# Observations that are the same at every timestep of a trajectory and large (pre-computed text features: 1.5 MB per
# timestep): trainers.TrajectoryStore keeps them ONCE, as a (1, ...) record, and every collate step repeats them over the
# trajectory's timesteps (`expand_once_records`).
ONCE_KEYS = ("rxr_instruction",)


def expand_once_records(obs: Dict, steps: int) -> Dict:
    """A trajectory's observations as the store returns them -> every `ONCE_KEYS` entry held as a (1, ...) record becomes a
    (steps, ...) view of it (no copy): what the collate steps pad and stack like any other observation."""
    out = obs
    for k in ONCE_KEYS:
        v = obs.get(k)
        if v is not None and v.shape[0] == 1 and steps > 1:
            if out is obs:
                out = dict(obs)
            out[k] = v.expand(steps, *v.shape[1:])
    return out


def dedupe_instruction_features(observations: Dict, first_rows: int, key: str = "rxr_instruction") -> Dict:
    """`dedupe_instructions` for pre-computed text features (INSTRUCTION_ENCODER.sensor_uuid "rxr_instruction"): a HOST-side
    collated time-major (T*N, L, E) float batch, `first_rows` = N trajectories.  collate_fn repeats a trajectory's features
    at every timestep and pads finished trajectories with 1.0 (dagger_trainer.py:66-70), so row (t, n) maps to n when it
    equals row (0, n) bit for bit and to N when it is all ones; adds `<key>_unique` (N + 1, L, E) - the t = 0 rows and the
    padding row - and `<key>_index` (T*N,), which the policies consume like the token pair.  The batch is left alone when
    any row is neither (or it is on the device, or T < 2).  Two elementwise compares over the batch: no sort or
    `torch.unique` over rows that are hundreds of thousands of floats wide."""
    t = observations.get(key)
    N = int(first_rows)
    if (t is None or not torch.is_tensor(t) or t.is_cuda or t.dim() != 3 or t.dtype != torch.float32 or N < 1
            or t.shape[0] % N != 0 or t.shape[0] < 2 * N):
        return observations
    T, L, E = t.shape[0] // N, t.shape[1], t.shape[2]
    bits = t.contiguous().view(torch.int32).view(T, N, L * E)
    same = (bits == bits[:1]).all(dim=2)                                              # (T, N): row (t, n) is row (0, n)
    pad = (bits == torch.ones((), dtype=torch.float32).view(torch.int32)).all(dim=2)  # (T, N): collate_fn's padding row
    if not bool((same | pad).all()):
        return observations
    index = torch.arange(N, dtype=torch.int32).expand(T, N).clone()
    index[~same] = N
    observations = dict(observations)
    observations[key + "_unique"] = torch.cat([t[:N], torch.ones((1, L, E), dtype=torch.float32)], 0).contiguous()
    observations[key + "_index"] = index.reshape(-1).contiguous()
    return observations


def add_batched_data_to_observations(observations: List[Dict], batched_data, batched_data_key: str):
    if batched_data is not None:
        for i in range(len(observations)):
            observations[i][batched_data_key] = batched_data[i]
    return observations
