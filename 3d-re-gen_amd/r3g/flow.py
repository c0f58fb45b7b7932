"""Sigma tables of the shape model's flow-matching samplers (host arithmetic, a few dozen floats) -- what upstream's schedulers
compute in `set_timesteps`.  The tables are handed to r3g_flow_sample_sigmas (include/r3g.h) as `steps + 1` float32 values; step i
evaluates the model at t = sigmas[i] and moves the latents by (sigmas[i + 1] - sigmas[i]) v.

[UPSTREAM-RECALLED] (no upstream source was at hand):
  FlowMatchEulerDiscreteScheduler            sigmas = linspace(0, 1, N), shifted, + a trailing 1 (the last step has d_sigma = 0)
  ConsistencyFlowMatchEulerDiscreteScheduler the turbo checkpoints' scheduler (num_train_timesteps 1000, pcm_timesteps 100):
      full  = linspace(0, 1, 1000)
      euler = [0] + (arange(1, pcm) * (1000 // pcm)).round() - 1          # 0, 9, 19, ..., 989
      idx   = floor(linspace(0, pcm, N, endpoint=False))
      sigmas = full[euler[idx]] ++ [1.0]
  no step of it has d_sigma = 0: N steps are N evaluations.
"""
import numpy as np

SCHEDULERS = ("FlowMatchEulerDiscreteScheduler", "ConsistencyFlowMatchEulerDiscreteScheduler")


def euler_sigmas(num_inference_steps, shift=1.0):
    """FlowMatchEulerDiscreteScheduler.set_timesteps(sigmas=linspace(0, 1, N)) -> float32 [N + 1], last = 1"""
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("num_inference_steps must be >= 1")
    s = np.linspace(0, 1, n)
    s = shift * s / (1 + (shift - 1) * s)
    return np.concatenate([s.astype(np.float32), np.ones(1, np.float32)])


def consistency_sigmas(num_inference_steps, num_train_timesteps=1000, pcm_timesteps=100):
    """ConsistencyFlowMatchEulerDiscreteScheduler.set_timesteps(N) -> float32 [N + 1], last = 1"""
    n, T, pcm = int(num_inference_steps), int(num_train_timesteps), int(pcm_timesteps)
    if n < 1:
        raise ValueError("num_inference_steps must be >= 1")
    if pcm < 1 or T < pcm:
        raise ValueError("pcm_timesteps must lie in [1, num_train_timesteps]")
    full = np.linspace(0, 1, T)
    euler = np.concatenate([np.zeros(1), (np.arange(1, pcm) * (T // pcm)).round() - 1]).astype(np.int64)
    idx = np.floor(np.linspace(0, pcm, n, endpoint=False)).astype(np.int64)
    return np.concatenate([full[euler[idx]].astype(np.float32), np.ones(1, np.float32)])


def explicit_sigmas(sigmas, shift=1.0):
    """the `sigmas=` keyword of the pipeline call: a strictly ascending table inside [0, 1] gets the scheduler's shift and the
    trailing 1, as upstream's set_timesteps(sigmas=...) does; anything else is a ValueError"""
    try:
        s = np.asarray(sigmas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sigmas: a 1-D sequence of numbers expected")
    if s.ndim != 1 or s.size < 1:
        raise ValueError("sigmas: a non-empty 1-D sequence expected")
    if not np.isfinite(s).all():
        raise ValueError("sigmas: every value must be finite")
    if s[0] < 0.0 or s[-1] > 1.0:
        raise ValueError("sigmas: values must lie in [0, 1] (the table ends below or at 1; the trailing 1 is added here)")
    if (np.diff(s) <= 0).any():
        raise ValueError("sigmas: the table must be strictly ascending")
    s = shift * s / (1 + (shift - 1) * s)
    return np.concatenate([s.astype(np.float32), np.ones(1, np.float32)])


def scheduler_sigmas(sched, num_inference_steps, sigmas=None):
    """the table of a pipeline call from its scheduler settings (cfg["sched"]: kind, shift, num_train_timesteps, pcm_timesteps)"""
    kind = sched.get("kind", SCHEDULERS[0])
    if kind not in SCHEDULERS:
        raise ValueError("scheduler %r is not one of %s" % (kind, ", ".join(SCHEDULERS)))
    if kind == SCHEDULERS[1]:
        if sigmas is not None:
            return explicit_sigmas(sigmas)
        return consistency_sigmas(num_inference_steps, sched.get("num_train_timesteps", 1000), sched.get("pcm_timesteps", 100))
    if sigmas is not None:
        return explicit_sigmas(sigmas, sched.get("shift", 1.0))
    return euler_sigmas(num_inference_steps, sched.get("shift", 1.0))
