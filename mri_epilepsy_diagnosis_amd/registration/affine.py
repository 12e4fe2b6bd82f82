"""Host side of the affine registration, float64 and deterministic: the 12-parameter transform between two voxel grids, the change
of a matrix between pyramid levels, and the batched pattern search that proposes candidate matrices.  Nothing here touches the
device; `optimise` sees the cost only through a callable, so the device kernels and a CPU reference can both drive it.

A matrix is a (3, 4) float64 array that maps a FIXED voxel index (d, h, w) to a MOVING voxel index, the convention of
`segmentation.transforms.warp3d` and of csrc/register.hip."""
import numpy as np

# a voxel this far from the centre moves by the translation step when a rotation, log-scale or shear parameter takes its step
LEVER = 80.0
DOF_CHOICES = (3, 6, 9, 12)


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def params_to_matrix(params, fixed_shape, moving_shape, fixed_spacing=(1, 1, 1), moving_spacing=(1, 1, 1)):
    """The (3, 4) fixed-voxel -> moving-voxel matrix of up to 12 parameters (missing ones are 0):
        translation (3, in units of the spacings), rotation about the three axes (3, radians), log-scale (3), shear (3).
    With p_f = S_f (o - c_f) the fixed voxel in physical units about the fixed grid's centre c_f = (N_f - 1) / 2:
        p_m = R * Shear * Scale * p_f + t,      moving voxel = S_m^-1 p_m + c_m.
    So rotation is about the fixed grid's centre and zero parameters map centre to centre."""
    p = np.zeros(12)
    params = np.asarray(params, dtype=np.float64).ravel()
    if params.size > 12:
        raise ValueError("params_to_matrix: at most 12 parameters, got %d" % params.size)
    p[:params.size] = params
    sf, sm = np.asarray(fixed_spacing, dtype=np.float64), np.asarray(moving_spacing, dtype=np.float64)
    if sf.shape != (3,) or sm.shape != (3,) or not (sf > 0).all() or not (sm > 0).all():
        raise ValueError("params_to_matrix: spacings must be three positive numbers, got %r and %r" % (fixed_spacing, moving_spacing))
    cf = (np.asarray(fixed_shape, dtype=np.float64) - 1) / 2
    cm = (np.asarray(moving_shape, dtype=np.float64) - 1) / 2
    shear = np.array([[1, p[9], p[10]], [0, 1, p[11]], [0, 0, 1]])
    lin = _rotation(p[3], p[4], p[5]) @ shear @ np.diag(np.exp(p[6:9]))
    M = np.diag(1 / sm) @ lin @ np.diag(sf)
    return np.concatenate([M, (cm + p[:3] / sm - M @ cf)[:, None]], axis=1)


def _square(m):
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (3, 4):
        raise ValueError("expected a (3, 4) matrix, got shape %s" % (m.shape,))
    return np.concatenate([m, [[0, 0, 0, 1]]], axis=0)


def invert(matrix):
    """The (3, 4) matrix of the inverse map (moving voxel -> fixed voxel)."""
    return np.linalg.inv(_square(matrix))[:3]


def compose(outer, inner):
    """The (3, 4) matrix of x -> outer(inner(x))."""
    return (_square(outer) @ _square(inner))[:3]


def level_matrix(matrix, fixed_level, moving_level=None):
    """A level-0 matrix between the grids of two pyramid levels.  Voxel o of level l sits at 2^l o + (2^l - 1) / 2 of level 0 (the
    centre of its cell of 2^l voxels), so the level matrix is U_m^-1 * matrix * U_f."""
    moving_level = fixed_level if moving_level is None else moving_level
    ff, fm = 2.0 ** fixed_level, 2.0 ** moving_level
    Uf = np.array([[ff, 0, 0, (ff - 1) / 2], [0, ff, 0, (ff - 1) / 2], [0, 0, ff, (ff - 1) / 2]])
    Um_inv = np.array([[1 / fm, 0, 0, -(fm - 1) / 2 / fm], [0, 1 / fm, 0, -(fm - 1) / 2 / fm], [0, 0, 1 / fm, -(fm - 1) / 2 / fm]])
    return compose(Um_inv, compose(matrix, Uf))


def corner_displacement(a, b, fixed_shape):
    """Mean distance, in moving voxels, between the images of the fixed grid's 8 corners under two matrices."""
    d, h, w = (float(s) - 1 for s in fixed_shape)
    corners = np.array([[x, y, z, 1.0] for x in (0, d) for y in (0, h) for z in (0, w)])
    diff = corners @ (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).T
    return float(np.sqrt((diff ** 2).sum(1)).mean())


def step_vector(step, dof):
    """Per-parameter steps for a translation step of `step`: rotation, log-scale and shear steps move a voxel LEVER voxels from the
    centre by the same distance.  Parameters beyond `dof` get 0."""
    s = np.zeros(12)
    s[:3] = step
    s[3:] = step / LEVER
    s[dof:] = 0
    return s


def optimise(evaluate, x0, dof, steps, tol, to_matrix, line=(0.5, 1.0, 2.0, 3.0), max_iter=200):
    """Batched pattern search over the first `dof` of 12 parameters.
        evaluate(list of (3, 4) matrices) -> sequence of costs (lower is better, +inf allowed)
        to_matrix(parameter vector) -> (3, 4) matrix
        steps: the 12 per-parameter steps to begin with (`step_vector`); tol: stop once the translation step is below it.
    One iteration scores the 2 * dof axis moves in ONE call of `evaluate`, combines the improving direction of every axis into one
    move, and scores the multiples `line` of it in a second call.  The best point seen becomes the new centre; when nothing
    improves the steps are halved.  Returns (parameters, cost, info) with info = {iterations, calls, evaluations}."""
    if dof not in DOF_CHOICES:
        raise ValueError("optimise: dof must be one of %s, got %r" % (DOF_CHOICES, dof))
    x = np.zeros(12)
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    x[:x0.size] = x0
    steps = np.array(steps, dtype=np.float64)
    info = {"iterations": 0, "calls": 0, "evaluations": 0}

    def score(points):
        info["calls"] += 1
        info["evaluations"] += len(points)
        costs = np.asarray(evaluate([to_matrix(p) for p in points]), dtype=np.float64)
        return np.where(np.isnan(costs), np.inf, costs)
    fx = float(score([x])[0])
    while steps[0] >= tol and info["iterations"] < max_iter:
        info["iterations"] += 1
        points = []
        for i in range(dof):
            for sign in (1.0, -1.0):
                p = x.copy()
                p[i] += sign * steps[i]
                points.append(p)
        costs = score(points)
        move = np.zeros(12)
        for i in range(dof):
            up, down = costs[2 * i], costs[2 * i + 1]
            if min(up, down) < fx:
                move[i] = steps[i] if up <= down else -steps[i]
        best = int(np.argmin(costs))
        best_x, best_f = (points[best], float(costs[best])) if costs[best] < fx else (x, fx)
        if np.count_nonzero(move) > 0:
            lpoints = [x + m * move for m in line]
            lcosts = score(lpoints)
            lb = int(np.argmin(lcosts))
            if lcosts[lb] < best_f:
                best_x, best_f = lpoints[lb], float(lcosts[lb])
        if best_f < fx:
            x, fx = best_x, best_f
        else:
            steps = steps / 2
    return x, fx, info
