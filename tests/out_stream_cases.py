"""What the lx_out tests share (tests/test_out_stream_abi.py on the host, tests/test_gpu_out_stream.py on the device): a record list
cut into pieces of whole query groups, each piece with its own query names, letters offsets and LCA pairs, its records' n_qid
counted within the piece -- what a front end that searches the queries block by block hands to lx_out_append."""
import ctypes as C

import numpy as np

from lambda_amd import capi


def lca_pairs(opt):
    """The (n_qid, taxon) pairs an options block points to, as arrays (empty without taxonomy)."""
    if not opt or not opt.n_lca:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    return (np.ctypeslib.as_array(C.cast(opt.lca_qid, C.POINTER(C.c_uint64)), (opt.n_lca,)).copy(),
            np.ctypeslib.as_array(C.cast(opt.lca_tax, C.POINTER(C.c_uint32)), (opt.n_lca,)).copy())


def piece(m, names, qoff, lca, q0, q1):
    """The records of the queries [q0, q1) as a list of its own."""
    lo, hi = np.searchsorted(m["n_qid"], [q0, q1])
    part = m[lo:hi].copy()
    part["n_qid"] -= q0
    part["qry_id"] = part["n_qid"]
    keep = (lca[0] >= q0) & (lca[0] < q1)
    return dict(bms=part, q_ids=names["q_ids"][q0:q1], q_lens=names["q_lens"][q0:q1], q_ascii_off=qoff[q0:q1],
                lca_qid=lca[0][keep] - np.uint64(q0), lca_tax=lca[1][keep])


def write_in_pieces(handle, path, fmt, case, opt, cuts, where, program="blastn", bgzf=False, footer=-1):
    """The file lx_out makes of the case's list cut at the query numbers `cuts` (equal neighbours: an empty piece); where: one
    LX_RENDER_* for all pieces, or one per piece."""
    m, ops, names, qa, qoff = case
    lca = lca_pairs(opt)
    bounds = [0] + list(cuts) + [len(names["q_ids"])]
    wheres = where if isinstance(where, (list, tuple)) else [where] * (len(bounds) - 1)
    with capi.Out(handle, path, fmt, names["s_ids"], names["s_lens"], program=program, bgzf=bgzf, options=opt) as out:
        for w, q0, q1 in zip(wheres, bounds, bounds[1:]):
            p = piece(m, names, qoff, lca, q0, q1)
            out.append(w, p["bms"], ops, p["q_ids"], p["q_lens"], q_ascii=qa, q_ascii_off=p["q_ascii_off"], lca_qid=p["lca_qid"], lca_tax=p["lca_tax"])
        out.close(footer)
    return path.read_bytes()
