"""gs_pose_step (csrc/pose_step.hip, include/gs_abi.h) restated in Python floats: explicit scalar operations, no NumPy
arithmetic and no BLAS, every sum left to right in the kernel's order.  A Python float is an IEEE double and the kernel is
built without contraction, so the two follow each other operation by operation; sqrt, sin, cos and the power of the bias
corrections are each library's own (a last-bit matter).

    state = new_state(rot, tran)                      # what gs_pose_reset writes
    row = step(state, grad_rot, grad_tran, values, opts, log_row, skip=False)
        # the log row (a list of floats); ``state`` is updated in place, state["pose32"] is what pose_dev holds afterwards
"""
import math
import struct


def f32(x: float) -> float:
    """``x`` rounded to float32 once (and back: the value pose_dev holds)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def new_state(rot, tran):
    R = [float(x) for row in rot for x in (row if hasattr(row, "__len__") else [row])]
    t = [float(x) for x in tran]
    assert len(R) == 9 and len(t) == 3
    return {"R": R, "t": t, "m": [0.0] * 6, "v": [0.0] * 6, "best_R": list(R), "best_t": list(t), "best_loss": math.inf,
            "steps": 0, "best_row": -1, "skipped": 0, "bad": 0, "pose32": [f32(x) for x in R + t]}


def default_opts(**kw):
    o = {"lr_rot": 2e-3, "lr_tran": 2e-3, "lr_scale": 1.0, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "track_best": 1,
         "n_values": 4}
    o.update(kw)
    return o


def tangent_grad(G, R):
    """dL/dw at w = 0 of exp([w]x) R from G = dL/dR: M = G R^T, (M21 - M12, M02 - M20, M10 - M01)."""
    M = [0.0] * 9
    for i in range(3):
        for j in range(3):
            M[3 * i + j] = G[3 * i] * R[3 * j] + G[3 * i + 1] * R[3 * j + 1] + G[3 * i + 2] * R[3 * j + 2]
    return [M[7] - M[5], M[2] - M[6], M[3] - M[1]]


def so3_exp(w0, w1, w2):
    """exp([w]x), row-major (Rodrigues; the series I + K + K K / 2 below 1e-8 rad)."""
    th = math.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    K = [0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0]
    KK = [0.0] * 9
    for i in range(3):
        for j in range(3):
            KK[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]
    ca, cb = 1.0, 0.5
    if not th < 1e-8:
        ca = math.sin(th) / th
        cb = (1.0 - math.cos(th)) / (th * th)
    return [((1.0 if k % 4 == 0 else 0.0) + ca * K[k]) + cb * KK[k] for k in range(9)]


def step(state, grad_rot, grad_tran, values, opts, log_row: int, skip: bool = False):
    """One gs_pose_step.  ``grad_rot`` [9], ``grad_tran`` [3], ``values`` [n_values]: the float32 inputs as Python floats."""
    G = [float(x) for x in grad_rot]
    gt = [float(x) for x in grad_tran]
    vals = [float(x) for x in values]
    assert len(G) == 9 and len(gt) == 3 and len(vals) == opts["n_values"]
    row = list(state["pose32"]) + G + gt + vals
    if skip:
        state["skipped"] += 1
        row[24] = math.nan
        return row
    if not all(math.isfinite(x) for x in G + gt + vals[:1]):
        state["bad"] += 1
        return row
    R, t = list(state["R"]), list(state["t"])
    loss = vals[0]
    if opts["track_best"] and loss < state["best_loss"]:
        state["best_R"], state["best_t"], state["best_loss"], state["best_row"] = list(R), list(t), loss, log_row
    g = tangent_grad(G, R) + gt
    state["steps"] += 1
    b1, b2 = opts["beta1"], opts["beta2"]
    bc1 = 1.0 - math.pow(b1, float(state["steps"]))
    bc2 = 1.0 - math.pow(b2, float(state["steps"]))
    d = [0.0] * 6
    for k in range(6):
        lr = (opts["lr_rot"] if k < 3 else opts["lr_tran"]) * opts["lr_scale"]
        m = b1 * state["m"][k] + (1.0 - b1) * g[k]
        v = b2 * state["v"][k] + ((1.0 - b2) * g[k]) * g[k]
        state["m"][k], state["v"][k] = m, v
        d[k] = (lr * (m / bc1)) / (math.sqrt(v / bc2) + opts["eps"])
    E = so3_exp(-d[0], -d[1], -d[2])
    Rn = [0.0] * 9
    for i in range(3):
        for j in range(3):
            Rn[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j]
    tn = [t[k] - d[3 + k] for k in range(3)]
    state["R"], state["t"] = Rn, tn
    state["pose32"] = [f32(x) for x in Rn + tn]
    return row
