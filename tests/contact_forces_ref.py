"""NumPy restatement of the (16,) record of `tacex_fem_contact_forces` from per-vertex forces of oracle/fem_oracle.py: what the GPU tests
of tests/test_contact_forces_gpu.py compare the kernel's record with.  Pinned on a closed-form case in tests/test_contact_forces.py."""
import numpy as np

from oracle.fem_oracle import ContactModel, FrictionModel, contact_distance

SLOTS = dict(normal_force=slice(0, 3), friction_force=slice(3, 6), torque=slice(6, 9), normal_magnitude=9, contact_area=10,
             num_contacts=11, centre_of_pressure=slice(12, 15), min_gap=15)


def normal_forces(area, ind, dhat, kappa, dt, x, mesh=None):
    """(V,3) barrier force ON the pad in newtons: -ContactModel.gradient / dt^2; and the signed distances (V,)."""
    cm = ContactModel(area, ind, dhat, kappa, dt, mesh)
    d, _ = contact_distance(np.asarray(ind, np.float64), x, mesh)
    with np.errstate(invalid="ignore"):
        return -cm.gradient(x) / dt**2, d


def friction_forces(area, ind_prev, dhat, kappa, dt, x_prev, disp, mu, eps_velocity, x, mesh=None):
    """(V,3) lagged friction force ON the pad in newtons, IPC's lag (the previous configuration): -FrictionModel.gradient / dt^2; and the
    model (its `lam`, `eps`, `_u` tell sticking from slipping vertices)."""
    fr = FrictionModel(ContactModel(area, ind_prev, dhat, kappa, dt, mesh), x_prev, disp, mu, eps_velocity)
    return -fr.gradient(x) / dt**2, fr


def kernel_order_sum(vals):
    """Sum of per-vertex values (V,) in the kernel's order: thread t of 256 adds its vertices t, t + 256, ... in ascending order, a wave
    adds its 64 lanes by the butterfly a[i] += a[i ^ s] for s = 32, 16, ... 1 (every lane ends with the same bits), the four waves are
    added in wave order.  Pure additions: bit for bit what the kernel computes for a slot whose terms are exact (the contact area)."""
    v = np.asarray(vals, np.float64)
    v = np.concatenate([v, np.zeros(-len(v) % 256)]).reshape(-1, 256)
    acc = np.zeros(256)
    for row in v:
        acc = acc + row
    a = acc.reshape(4, 64)
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ s]
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def wrench_record(x, f_n, f_f, area, d, dhat, ref):
    """The 16 slots from per-vertex forces f_n, f_f (V,3) at positions x (V,3), vertex weights `area` (V,), signed distances d (V,):
    0..2 sum f_n | 3..5 sum f_f | 6..8 sum (x - ref) x (f_n + f_f) | 9 sum |f_n| | 10 area of the active vertices (summed in the kernel's order: exact) | 11 their number |
    12..14 sum |f_n| x / sum |f_n| (ref without contact) | 15 smallest gap over the surface vertices (+inf: none)."""
    x, f_n, f_f, ref = (np.asarray(a, np.float64) for a in (x, f_n, f_f, ref))
    surf = np.asarray(area) > 0
    act = surf & (d > 0) & (d < dhat)
    lam = np.linalg.norm(f_n, axis=1)
    r = np.zeros(16)
    r[0:3], r[3:6] = f_n.sum(0), f_f.sum(0)
    r[6:9] = np.cross(x - ref, f_n + f_f).sum(0)
    r[9], r[10], r[11] = lam.sum(), kernel_order_sum(np.where(act, area, 0.0)), act.sum()
    r[12:15] = ref + (lam[:, None] * (x - ref)).sum(0) / lam.sum() if lam.sum() > 0 else ref
    ds = d[surf & np.isfinite(d)]
    r[15] = ds.min() if len(ds) else np.inf
    return r
