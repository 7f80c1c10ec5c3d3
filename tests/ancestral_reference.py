"""An exact host reference of the marginal ancestral states of one (node, other, matrix) triple, for tests only.

    a[n][i] = sum_r w_r pi_r[i] node[n, r, i] * sum_j P_r[i][j] other[n, r, j],      probs[n][i] = a[n][i] / sum_i a[n][i]

(src/tree/treeinfo.c:1698; scaler counts and p-inv ignored, a row whose sum is 0 stays all zero), evaluated in
numpy.longdouble from what the library under test holds: its own vectors (a coded tip as the 0/1 expansion of its
masks), its own P-matrix, the frequencies of params_indices[r] and the rate weights of the partition.  The inputs
being the engine's doubles, an engine differs from this table only by the fp64 rounding of sums of non-negative terms:

    |got - ref| <= 2 (R S + S + 8) 2^-53 ref + 2^-1000

R S additions in the two nested sums, S in the row sum, 8 for the constant factors and the division, a factor 2 of
margin; the absolute term lets products that underflow to 0 in fp64 pass."""
import numpy as np

import pllhip_ctypes as pc

LD = np.longdouble


def clv_of(inst, idx):
    """[site][rate][state] doubles of a vector as the engine holds it.  The oracle keeps a coded tip as codes only
    (tipchars / tipmap): those are expanded here; the product's pllhip_get_clv expands them itself."""
    p = inst.p.contents
    if not inst.lib.is_product and (p.attributes & pc.PLL_ATTRIB_PATTERN_TIP) and idx < inst.tips:
        chars = np.ctypeslib.as_array(p.tipchars[idx], shape=(inst.N,))
        masks = np.array([int(p.tipmap[int(c)]) for c in chars], dtype=object)
        bits = np.array([[(int(m) >> j) & 1 for j in range(inst.S)] for m in masks], dtype=np.float64)
        return np.repeat(bits[:, None, :], inst.R, axis=1)
    return inst.get_clv(idx)


def model_of(inst):
    """(frequencies [rate][state] of params_indices[r], rate weights [rate]) from the partition's own arrays"""
    p = inst.p.contents
    freqs = np.array([[p.frequencies[int(inst.params[r])][i] for i in range(inst.S)] for r in range(inst.R)])
    weights = np.array([p.rate_weights[r] for r in range(inst.R)])
    return freqs, weights


def table(node, other, pmatrix, freqs, weights):
    """probs [site][state] in longdouble; node / other [site][rate][state], pmatrix [rate][state][state],
    freqs [rate][state], weights [rate]"""
    node, other, P = np.asarray(node, dtype=LD), np.asarray(other, dtype=LD), np.asarray(pmatrix, dtype=LD)
    pi, w = np.asarray(freqs, dtype=LD), np.asarray(weights, dtype=LD)
    N, R, S = node.shape
    a = np.zeros((N, S), dtype=LD)
    for r in range(R):
        t = np.zeros((N, S), dtype=LD)
        for j in range(S):                                  # t[n][i] = sum_j P_r[i][j] other[n, r, j]
            t += other[:, r, j:j + 1] * P[r, :, j][None, :]
        a += w[r] * pi[r][None, :] * node[:, r, :] * t
    total = a.sum(axis=1, keepdims=True)
    return np.divide(a, total, out=np.zeros_like(a), where=total > 0)


def reference(inst, node, other, matrix):
    """the table of one triple from what `inst` holds"""
    freqs, weights = model_of(inst)
    return table(clv_of(inst, node), clv_of(inst, other), inst.get_pmatrix(matrix), freqs, weights)


def bound(ref, rate_cats, states):
    """the derived bound per entry (longdouble)"""
    return LD(2 * (rate_cats * states + states + 8)) * LD(2.0) ** -53 * ref + LD(2.0) ** -1000


def worst_fraction(got, ref, rate_cats, states):
    """largest |got - ref| as a fraction of the bound"""
    got = np.asarray(got, dtype=LD)
    return float(np.max(np.abs(got - ref) / bound(ref, rate_cats, states))) if got.size else 0.0


def clear_rows(ref, rate_cats, states):
    """(clear, zero): rows whose two largest reference values differ by more than the bounds of both -- an engine
    within the bound has to name the reference's state there -- and rows that are all zero (state 0, probability 0)"""
    if ref.shape[1] == 1:
        return np.ones(len(ref), dtype=bool), ref[:, 0] == 0
    top = np.sort(ref, axis=1)
    b = bound(top, rate_cats, states)
    zero = top[:, -1] == 0
    return (top[:, -1] - top[:, -2] > b[:, -1] + b[:, -2]) & ~zero, zero
