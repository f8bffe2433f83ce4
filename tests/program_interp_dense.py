"""Interpreter of HTTP device programs with dense automata (TEST INFRA).

program_interp.HttpProgram with the walk of program.h kDfaDense (dfa_pack.h
DenseDfa): per byte the class map -- its LDS-image copy where the kernel
reads that one (DfaDesc::lds_cmap) --, then one u16 entry of the table,
T16[state * ncls + class].  End codes, sets and candidate entries are the
packed kind's, so everything else is the base class."""
import numpy as np

from program_interp import DFA_FIELDS, DFA_WORDS, KNONE, LATCHED, HttpProgram

DFA_DENSE = 3  # program.h kDfaDense
LDS_CMAP_WORD = len(DFA_FIELDS)  # DfaDesc::lds_cmap follows lds_mid


class DenseHttpProgram(HttpProgram):
    def __init__(self, prog: np.ndarray):
        super().__init__(prog)
        self.prog16 = self.prog.view(np.uint16)
        assert LDS_CMAP_WORD == 30 and DFA_WORDS == 32
        for k, d in enumerate(self.dfas):
            d["lds_cmap"] = self.img[self.h["lds_dfas"] + DFA_WORDS * k + LDS_CMAP_WORD]

    @property
    def dense_dfas(self):
        return [k for k, d in enumerate(self.dfas) if d["kind"] == DFA_DENSE]

    def cmap(self, d) -> bytes:
        """The class map the kernel reads: the LDS copy when there is one
        (which must equal the program's)."""
        g = self.prog_bytes[4 * d["acc_cmap_off"]: 4 * d["acc_cmap_off"] + 256]
        if d["lds_cmap"] == KNONE:
            return g
        l = self.img_bytes[4 * d["lds_cmap"]: 4 * d["lds_cmap"] + 256]
        assert l == g
        return l

    def walk(self, k, data: bytes):
        d = self.dfas[k]
        if d["kind"] != DFA_DENSE:
            return super().walk(k, data)
        # what a dense descriptor must not have (program.h)
        assert d["lds_table"] == d["lds_es"] == d["lds_latch"] == d["lds_skip"] == d["lit_tab"] == KNONE
        assert d["n_slots"] == d["nstates"] * d["acc_ncls"] and 0 < d["acc_ncls"] <= 256
        assert d["nstates"] <= 65535
        cm = self.cmap(d)
        ncls, region, t0 = d["acc_ncls"], d["region"], 2 * d["table_off"]
        st, last = d["start_base"], KNONE
        for b in data:  # (no dead check: state 0 is an all-zero row)
            c = cm[b]
            assert c < ncls
            slot = st * ncls + c
            if st < region:
                last = slot
            st = int(self.prog16[t0 + slot])
            assert st < d["nstates"]
        if not st:
            return 0
        es = self.w[d["es_off"] + st]
        if es != LATCHED:
            return es
        return LATCHED | (d["start_latch"] if last == KNONE else self.w[d["latch_off"] + last])
