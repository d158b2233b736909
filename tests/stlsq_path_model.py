"""csrc/stlsq_path.hpp in numpy fp64, statement by statement: the model the GPU test compares symode_stlsq_path with.  The
row solve is ``tests.stlsq_cases.row_solve``, the restatement of csrc/stlsq.hpp that tests/test_host_stlsq_rows.py checks
against the host."""
import numpy as np

from tests.stlsq_cases import row_solve


def rss(H, p, j, sel, w):
    """stlsq_path_rss: lane k forms q_k over the support ascending and r_k; e starts at Hyy and takes r_k, k ascending."""
    r = {}
    for k in sel:
        q = 0.0
        for l in sel:
            q += H[k, l] * w[l]
        r[k] = w[k] * (q - 2.0 * H[k, p + j])
    e = H[p + j, p + j]
    for k in sel:
        e += r[k]
    return e


def smallest(active, av):
    """stlsq_path_smallest: (index, |v|) of the active column with the smallest fp32 |v|, the lowest index of equals."""
    bi, bv = None, None
    for k in range(len(av)):
        if active[k] and (bi is None or av[k] < bv):
            bi, bv = k, av[k]
    return bi, bv


def path(G, V, d, gamma, tol, floor_rel, near_band, n_problems=None):
    """stlsq_path_kernel for G (n_sets, p+d, p+d), V (n_val_sets, p+d, p+d).  A dict of the entry's outputs; a problem that
    fell keeps whatever it held when it ended (unspecified by the entry)."""
    n_sets, n_val_sets, p = G.shape[0], V.shape[0], G.shape[1] - d
    S = n_sets if n_problems is None else n_problems
    o = dict(path_xi=np.zeros((S, d, p + 1, p), dtype=np.float32), order=np.zeros((S, d, p), dtype=np.int32),
             rss_train=np.zeros((S, d, p + 1)), rss_val=np.zeros((S, d, p + 1)), best=np.zeros((S, d), dtype=np.int32),
             Xi=np.zeros((S, d, p), dtype=np.float32), mask=np.zeros((S, d, p), dtype=bool), near=np.zeros(S, dtype=np.int32),
             fell=np.zeros(S, dtype=np.int32))
    g2 = gamma * gamma
    for s in range(S):
        Gs, Vs = G[s % n_sets], V[s % n_val_sets]
        Gtt = Gs[:p, :p] + np.where(np.eye(p) > 0, g2, 0.0)
        rem = np.full((d, p), -1)
        # the rows of a problem step together (their "pivot not positive" flags meet after every solve)
        active = np.ones((d, p), dtype=bool)
        for t in range(p + 1):
            rows = []
            for j in range(d):
                sel = np.nonzero(active[j])[0]
                x = np.zeros(p)
                if len(sel):
                    w = row_solve(Gtt[np.ix_(sel, sel)], Gs[sel, p + j])
                    if w is None:
                        o['fell'][s] = 1
                        break
                    x[sel] = w
                rows.append((sel, x.astype(np.float32)))
            if o['fell'][s]:
                break
            for j, (sel, v) in enumerate(rows):
                o['path_xi'][s, j, t] = v
                w64 = v.astype(np.float64)
                o['rss_train'][s, j, t] = rss(Gs, p, j, sel, w64)
                o['rss_val'][s, j, t] = rss(Vs, p, j, sel, w64)
                if len(sel):
                    av = np.abs(v)
                    out, lo = smallest(active[j], av)
                    if len(sel) > 1:
                        rest = active[j].copy()
                        rest[out] = False
                        _, up = smallest(rest, av)
                        o['near'][s] += int(np.float64(up) - np.float64(lo) < near_band)
                    o['order'][s, j, t] = out
                    active[j, out] = False
                    rem[j, out] = t
        if o['fell'][s]:
            continue
        for j in range(d):
            ev, vyy = o['rss_val'][s, j], Vs[p + j, p + j]
            e_min = vyy
            for t in range(p):
                if ev[t] < e_min:
                    e_min = ev[t]
            cut = (1.0 + tol) * (e_min if e_min > 0.0 else 0.0) + floor_rel * vyy
            ok = [t for t in range(p) if ev[t] <= cut]
            best = p if (vyy <= cut or not ok) else ok[-1]
            m = rem[j] >= best
            sel = np.nonzero(m)[0]
            x = np.zeros(p)
            if len(sel):
                x[sel] = row_solve(Gtt[np.ix_(sel, sel)], Gs[sel, p + j])
            o['best'][s, j], o['Xi'][s, j], o['mask'][s, j] = best, x.astype(np.float32), m
    return o
