"""Big-integer model of the element-wise steps between the transforms (a plain helper module, imported by the step tests).

One function per launcher of apsu_amd/csrc/device.h, each written from the mathematical definition of the step on Python integers
(numpy object arrays, one entry per coefficient): the fast base conversion as an integer sum, SmMRq with the centred lift of r,
floor((x + half) / q_last) on the CRT value, fast_floor and fastbconv_sk with the centred alpha, the key-switch inner product and the
rounded division by p, round(m Q / t).  Nothing here knows a Shoup constant, a lazy range or a fold: the bodies are those of
oracle/pymodel.py (Model._extend, multiply, relinearize, mod_switch_to_next, add_plain) taken apart into steps, with the modular
inverses computed once per level.  tests/test_kernel_step_model_cpu.py composes the steps with the oracle's transforms and holds the
compositions to the C oracle, so a GPU mismatch (tests/test_gpu_kernel_steps.py) means the kernel.

RAW operands: the model's input is the raw word w; it stands for w n^-1 psi^-k mod m at coefficient k (StepModel.twist), psi being
this module's own minimal primitive 2n-th root.

Summed forms.  tensor_sum and i0_finish are the sums of the individually multiplied / rounded terms (exactly linear in what the kernel
gets as a sum, so the split of that sum over the terms does not matter: term 0 takes it).  finish_sum is stated on what the kernel
receives -- per-term q limbs and ONE set of Bsk limbs: the per-term scaled residues [t d (Q/q_j)^-1]_{q_j} enter the base conversion as
integers and are added there, the rest follows once.  "The sum of the individually finished terms" needs per-term Bsk limbs, which the
kernel never sees, and equals this only while every term's quotient lies inside fastbconv_sk's exact range; the CPU test shows the
equality on the products of real ciphertexts (finish_sum of the summed Bsk limbs == the sum of finish per term == the oracle).
"""
import numpy as np

from oracle import pymodel

MT = 1 << 32
W64 = 1 << 64


def O(a):
    """uint64 array -> array of Python integers"""
    return np.asarray(a).astype(object)


def U(a):
    return np.ascontiguousarray(np.asarray(a, dtype=object).astype(np.uint64))


def prod(xs):
    return pymodel.prod(xs)


class Level:
    """the moduli of one chain level and the inverses the definitions name"""

    def __init__(self, q, B, m_sk, t):
        self.q, self.B, self.m_sk, self.t = [int(v) for v in q], [int(v) for v in B], int(m_sk), int(t)
        self.L, self.nB = len(self.q), len(self.B)
        self.Bsk = self.B + [self.m_sk]
        self.ext = self.q + self.Bsk
        self.E = len(self.ext)
        self.Q, self.Bprod = prod(self.q), prod(self.B)
        self.punct_q = [self.Q // m for m in self.q]
        self.inv_punct_q = [pow(p, -1, m) for p, m in zip(self.punct_q, self.q)]
        self.punct_B = [self.Bprod // m for m in self.B]
        self.inv_punct_B = [pow(p, -1, m) for p, m in zip(self.punct_B, self.B)]
        self.invQ_mt = pow(self.Q, -1, MT)
        self.inv_mt = [pow(MT, -1, m) for m in self.Bsk]
        self.invQ = [pow(self.Q, -1, m) for m in self.Bsk]
        self.invB_msk = pow(self.Bprod, -1, self.m_sk)
        self.half = self.q[-1] >> 1

    def crt(self, limbs, base=None):
        """the value in [0, prod(base)) of canonical limbs [len(base)][n]"""
        base = self.q if base is None else base
        P = prod(base)
        x = 0
        for c, m in zip(limbs, base):
            x = x + c * pow(P // m, -1, m) % m * (P // m)
        return x % P


class StepModel:
    def __init__(self, n, key_q, t, levels):
        """levels: per chain index (q, B, m_sk)"""
        self.n, self.t = n, int(t)
        self.key_q = [int(v) for v in key_q]
        self.K = len(self.key_q)
        self.p = self.key_q[-1] if self.K > 1 else 0
        self.lv = [Level(q, B, m_sk, t) for q, B, m_sk in levels]
        self._tw = {}

    @classmethod
    def from_pymodel(cls, M):
        """the levels of oracle/pymodel.py's Model (SEAL's auxiliary base)"""
        levels = []
        for c in range(M.first + 1):
            q, _, B, m_sk, _ = M.rns_tool(c)
            levels.append((q, B, m_sk))
        return cls(M.n, M.key_q, M.t, levels)

    # ---- RAW words
    def twist_table(self, m):
        """n^-1 psi^-k mod m, k < n"""
        if m not in self._tw:
            ipsi = pow(pymodel.minimal_primitive_root(2 * self.n, m), -1, m)
            ninv = pow(self.n, -1, m)
            tab, w = [], ninv
            for _ in range(self.n):
                tab.append(w)
                w = w * ipsi % m
            self._tw[m] = np.array(tab, dtype=object)
        return self._tw[m]

    def twist(self, w, m):
        """the residue a raw word stands for"""
        return w * self.twist_table(m) % m

    def untwist(self, c, m, lift=0):
        """a raw word that stands for the canonical residue c: the smallest one, plus `lift` times m (kept below 2^64)"""
        inv = np.array([pow(int(v), -1, m) for v in self.twist_table(m)], dtype=object)
        w = c * inv % m + lift * m
        assert (w < W64).all()
        return w

    def canon(self, limbs, mods, raw):
        return [self.twist(x, m) if raw else x for x, m in zip(limbs, mods)]

    # ---- drop the last limb of a base with rounding: floor((x + half) / last) on the CRT value
    @staticmethod
    def drop_base(limbs, base):
        last, kept = base[-1], base[:-1]
        P = prod(base)
        x = 0
        for c, m in zip(limbs, base):
            x = x + c * pow(P // m, -1, m) % m * (P // m)
        y = (x % P + (last >> 1)) // last
        return [y % m for m in kept]

    def modswitch(self, c, poly, raw=False):
        """[L][n] at chain index c -> [L - 1][n]"""
        lv = self.lv[c]
        return self.drop_base(self.canon(poly, lv.q, raw), lv.q)

    # ---- BEHZ steps 1-2: q -> q u Bsk
    def ext_trace(self, c, poly):
        lv = self.lv[c]
        xs = [x * MT % m for x, m in zip(poly, lv.q)]
        y = 0
        for x, ip, pu, m in zip(xs, lv.inv_punct_q, lv.punct_q, lv.q):
            y = y + x * ip % m * pu                                     # fastbconv as an integer
        r = (-(y % MT) * lv.invQ_mt) % MT
        hi = (r >= MT // 2).astype(bool)
        out = []
        for m, imt in zip(lv.Bsk, lv.inv_mt):
            rc = np.where(hi, r + (m - MT), r)                          # centred lift of r into Z_m
            out.append((y % m + lv.Q * rc) * imt % m)
        return list(poly) + out, r

    def behz_ext(self, c, poly):
        """[L][n] canonical -> [E][n]"""
        return self.ext_trace(c, poly)[0]

    def drop_behz_ext(self, c, poly, raw=False):
        """[L + 1][n] at chain index c + 1 -> [E][n] at c"""
        return self.behz_ext(c, self.modswitch(c + 1, poly, raw))

    # ---- BEHZ step 4
    def tensor_conv(self, c, a, b):
        """a [sa][E][n], b [sb][E][n] -> [sa + sb - 1][E][n], every product reduced before the modular add"""
        lv = self.lv[c]
        sa, sb = len(a), len(b)
        out = []
        for I in range(sa + sb - 1):
            row = []
            for e, m in enumerate(lv.ext):
                acc = 0
                for i in range(max(0, I - (sb - 1)), min(I, sa - 1) + 1):
                    acc = (acc + a[i][e] * b[I - i][e] % m) % m
                row.append(acc)
            out.append(row)
        return out

    def tensor(self, c, a, b):
        return self.tensor_conv(c, a, b)

    def tensor_sum(self, c, a, b):
        """a, b [terms][2][E][n] -> (dq [terms][3][L][n], bs [3][nBsk][n]): the individually multiplied terms, their Bsk limbs summed"""
        lv = self.lv[c]
        per = [self.tensor_conv(c, x, y) for x, y in zip(a, b)]
        dq = [[d[p][:lv.L] for p in range(3)] for d in per]
        bs = [[sum(d[p][lv.L + i] for d in per) % m for i, m in enumerate(lv.Bsk)] for p in range(3)]
        return dq, bs

    # ---- BEHZ steps 6-8
    def finish_core(self, c, xq, xb):
        """xq [L]: integers entering fastbconv(q -> Bsk) per q limb; xb [nBsk]: t x mod Bsk_i -> (res [L][n], alpha)"""
        lv = self.lv[c]
        y = 0
        for x, pu in zip(xq, lv.punct_q):
            y = y + x * pu
        fl = [(b - y) * iq % m for b, iq, m in zip(xb, lv.invQ, lv.Bsk)]                 # fast_floor
        z = 0
        for f, ip, pu, m in zip(fl[:-1], lv.inv_punct_B, lv.punct_B, lv.B):
            z = z + f * ip % m * pu
        alpha = (z - fl[-1]) * lv.invB_msk % lv.m_sk
        alpha = np.where((alpha > lv.m_sk // 2).astype(bool), alpha - lv.m_sk, alpha)    # centred
        return [(z - alpha * lv.Bprod) % m for m in lv.q], alpha

    def scaled_q(self, c, dq):
        lv = self.lv[c]
        return [x * lv.t % m * ip % m for x, ip, m in zip(dq, lv.inv_punct_q, lv.q)]

    def finish_trace(self, c, d, raw=False):
        lv = self.lv[c]
        d = self.canon(d, lv.ext, raw)
        return self.finish_core(c, self.scaled_q(c, d[:lv.L]), [x * lv.t % m for x, m in zip(d[lv.L:], lv.Bsk)])

    def behz_finish(self, c, d, raw=False, acc=None):
        """d [terms][E][n] of one output polynomial -> [L][n] = (acc +) the sum of the finished terms"""
        lv = self.lv[c]
        out = [0] * lv.L if acc is None else list(acc)
        for term in d:
            res = self.finish_trace(c, term, raw)[0]
            out = [(o + r) % m for o, r, m in zip(out, res, lv.q)]
        return out

    def finish_sum_trace(self, c, dq, bs, raw=False):
        lv = self.lv[c]
        xq = [0] * lv.L
        for term in dq:
            s = self.scaled_q(c, self.canon(term, lv.q, raw))
            xq = [a + b for a, b in zip(xq, s)]                                           # integers, not residues
        bs = self.canon(bs, lv.Bsk, raw)
        return self.finish_core(c, xq, [x * lv.t % m for x, m in zip(bs, lv.Bsk)])

    def behz_finish_sum(self, c, dq, bs, raw=False):
        """dq [terms][L][n], bs [nBsk][n] of one output polynomial -> [L][n]"""
        return self.finish_sum_trace(c, dq, bs, raw)[0]

    # ---- key switching
    def acc_mods(self, c):
        return self.lv[c].q + [self.p]

    def ks_inner(self, c, tdec, rk):
        """tdec [L + 1][L][n], rk [K - 1][2][K][n] -> [2][L + 1][n]"""
        L = self.lv[c].L
        out = [[None] * (L + 1) for _ in range(2)]
        for I, m in enumerate(self.acc_mods(c)):
            ki = self.K - 1 if I == L else I
            for comp in range(2):
                out[comp][I] = sum(tdec[I][J] * rk[J][comp][ki] for J in range(L)) % m
        return out

    def ks_moddown(self, c, acc, ct, raw=False):
        """acc [2][L + 1][n], ct [2][L][n] -> ct + round(acc / p)"""
        mods = self.acc_mods(c)
        out = []
        for comp in range(2):
            y = self.drop_base(self.canon(acc[comp], mods, raw), mods)
            out.append([(x + v) % m for x, v, m in zip(ct[comp], y, self.lv[c].q)])
        return out

    # ---- evaluation tail
    def i0_finish(self, c, s, v, acc, raw=False, store=False):
        """c: the level before the drop.  s [L - 1][n], v [terms][n], acc [L - 1][n] of one polynomial -> [L - 1][n]"""
        lv = self.lv[c]
        kept = lv.q[:-1]
        s = self.canon(s, kept, raw)
        out = [0] * len(kept) if store else list(acc)
        for t, vt in enumerate(v):
            vt = self.twist(vt, lv.q[-1]) if raw else vt
            res = self.drop_base((s if t == 0 else [0 * vt] * len(kept)) + [vt], lv.q)
            out = [(o + r) % m for o, r, m in zip(out, res, kept)]
        return out

    def scale_plain(self, c, m):
        """round(m Q / t) per SEAL's add_plain: floor((m Q + floor((t + 1) / 2)) / t)"""
        lv = self.lv[c]
        return (m * lv.Q + (lv.t + 1) // 2) // lv.t

    def add_plain(self, c, c0, pt):
        s = self.scale_plain(c, pt)
        return [(x + s) % m for x, m in zip(c0, self.lv[c].q)]

    def lift(self, c, pt, no_lift=False):
        th = (self.t + 1) // 2
        up = (pt >= th).astype(bool) & (not no_lift)
        return [np.where(up, pt + (m - self.t), pt) for m in self.lv[c].q]

    def eval_epilogue(self, c, ct, a0, mask, add1=None, add2=None, clear_bits=0):
        """ct [2][L][n] -> [2][n]: addends, the two scaled plaintexts into c0, every limb dropped down to chain index 0, low bits cleared"""
        q = self.lv[c].q
        x = [[v for v in p] for p in ct]
        for add in (add1, add2):
            if add is not None:
                x = [[(u + w) % m for u, w, m in zip(p, ap, q)] for p, ap in zip(x, add)]
        x[0] = self.add_plain(c, self.add_plain(c, x[0], a0), mask)
        for l in range(c, 0, -1):
            x = [self.modswitch(l, p) for p in x]
        keep = ~((1 << clear_bits) - 1) if clear_bits > 0 else -1
        return [p[0] & (keep & (W64 - 1)) for p in x]
