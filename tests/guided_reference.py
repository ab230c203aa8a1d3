"""CPU reference of classifier-free guidance (include/movenet_hip.h, mvn_generate_guided), built on the
numpy ring oracle (oracle.wavenet_oracle.RingState.step) and the float64 references of the sampled choice
(tests/sampling_reference.py, tests/truncation_reference.py): two ring states -- contexts 0 and e -- the fp32 combine,
one choice, fed to both."""
import numpy as np

from oracle import wavenet_oracle as O

import sampling_reference as R
import truncation_reference as TR


def guided_logits(lc, lu, scales):
    """l = l_c + (s - 1) * (l_c - l_u) in fp32, in this order: subtract, multiply, add.  ``lc``, ``lu``: (..., Q)
    float32; ``scales``: a scalar or an array broadcast against their leading axes."""
    lc, lu = np.asarray(lc, np.float32), np.asarray(lu, np.float32)
    sm1 = (np.asarray(scales, np.float32) - np.float32(1.0)).astype(np.float32)
    sm1 = sm1.reshape(sm1.shape + (1,) * (lc.ndim - sm1.ndim))
    d = (lc - lu).astype(np.float32)
    m = (sm1 * d).astype(np.float32)
    return (lc + m).astype(np.float32)


def greedy_picks(lg):
    """The greedy rule of the generators: the first arg-max of softmax(softmax(l)); (..., Q) -> (...)."""
    flat = np.ascontiguousarray(lg, np.float32).reshape(-1, lg.shape[-1])
    return O._double_softmax_argmax(flat).reshape(lg.shape[:-1])


def top2_margin(lg):
    s = np.sort(np.asarray(lg, np.float64), axis=-1)
    return s[..., -1] - s[..., -2]


def sampled_picks(lg, temperature, top_k, top_p, uniform, sampling="model"):
    """float64 inverse-CDF picks of a sampled step over the (truncated) weights of ``lg``."""
    w = (TR.model_weights if sampling == "model" else TR.reference_weights)(lg, temperature)
    return R.inverse_cdf_picks(TR.truncated_cdf(w, TR.kept_set(w, top_k, top_p)), uniform)


def generate_guided(sd, dims, prompt_idx, n_total, ctx_c, scales, ctx_u=None, forced_idx=None, settings=None,
                    sampling="model"):
    """``prompt_idx`` (B, P >= 1); ``ctx_c`` / ``ctx_u`` (B, C) context vectors of the conditional / unconditional
    rows, constant in time (``ctx_u`` None: zeros).  ``settings``: None (greedy) or per pair (T, top_k, top_p, seed,
    row).  Returns (choices (B, n_total) -- the prompt, then the picks --, lu, lc, lg (B, n_total, Q) indexed by the time
    they predict, rows of times < 1 zero).  With ``forced_idx`` (B, n_total) the history fed back is teacher-forced."""
    prompt_idx = np.asarray(prompt_idx)
    B, P = prompt_idx.shape
    Q = dims.input_channels
    ctx_c = np.asarray(ctx_c, np.float32)
    ctx_u = np.zeros_like(ctx_c) if ctx_u is None else np.asarray(ctx_u, np.float32)
    su, sc = O.RingState(sd, dims, B), O.RingState(sd, dims, B)
    choices = np.zeros((B, n_total), np.int64)
    choices[:, :P] = prompt_idx
    lu, lc, lg = (np.zeros((B, n_total, Q), np.float32) for _ in range(3))
    for t in range(n_total - 1):
        fed = choices[:, t] if (forced_idx is None or t < P) else np.asarray(forced_idx)[:, t]
        u = t + 1
        lu[:, u], lc[:, u] = su.step(fed, ctx_u), sc.step(fed, ctx_c)
        lg[:, u] = guided_logits(lc[:, u], lu[:, u], scales)
        if u >= P:
            if settings is None:
                choices[:, u] = greedy_picks(lg[:, u])
            else:
                for b, (T, k, p, seed, row) in enumerate(settings):
                    if T > 0:
                        uni = R.philox_uniform(seed, np.array([[u]]), np.array([[row]]))
                        choices[b, u] = sampled_picks(lg[b:b + 1, u][None], T, k, p, uni, sampling)[0, 0]
                    else:
                        choices[b, u] = greedy_picks(lg[b:b + 1, u])[0]
    return choices, lu, lc, lg
