"""The rules of the IVF search with a filter, the caller's tables, the inner product and a radius (include/deltapq_amd.h
"IVF search: filters, caller tables, inner product and range search"), restated in numpy for tests/test_ivf_modes.py.  No
tests in here, and nothing but numpy.

Every answer is an existing rule applied to the eligible part of the union of the probed lists:
  eligibility   tests/_option_matrix.py eligible(): by reported id r, r < len(mask) and mask[r], the even-N rule applied;
  top-k         tests/_candidates_restatement.py search_row() over tests/_ivf_restatement.py union() cut to the eligible ids;
  tables, IP    tests/_tables_restatement.py (distances_dtc / distances_plain, ip_tables, ip_scores);
  coarse IP     tests/_exact_ip_restatement.py over the centroids;
  range         tests/_numeric_edges.py range_list()'s rule over the eligible union.
id rules: id_base, n_local, n_total, even_rule of _candidates_restatement.search_row.
"""
import numpy as np

import _candidates_restatement as C
import _exact_ip_restatement as EI
import _ivf_restatement as R
import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as T


def _rules(n, id_base=0, n_local=None, n_total=None, even_rule=True):
    n_local = n if n_local is None else n_local
    n_total = id_base + n_local if n_total is None else n_total
    return id_base, n_local, n_total, even_rule


def _renaming_total(n_total, even_rule):
    """The N_total _option_matrix's id functions take: they rename the last node of an even total, which a handle
    without the even-N rule (dpq_open_plain_*) never does -- an odd number stands for "no renaming"."""
    return n_total if even_rule else n_total | 1


def eligible_ids(mask, n, **id_rules):
    """int64, ascending: the reported ids of the handle's nodes the filter allows (mask: bool over reported ids; None:
    every node)."""
    id_base, n_local, n_total, even_rule = _rules(n, **id_rules)
    N = _renaming_total(n_total, even_rule)
    if mask is None:
        return om.reported_ids(np.arange(n_local), id_base, N)
    return om.eligible(np.asarray(mask, dtype=bool), n_local, base=id_base, N_total=N)[1]


def eligible_union(offsets, ids, probes_row, mask, n, **id_rules):
    """int64, ascending: the ids of the lists one query probes that the filter allows."""
    u = np.sort(R.union(offsets, ids, probes_row))
    return u if mask is None else u[np.isin(u, eligible_ids(mask, n, **id_rules))]


def search_row(d, offsets, ids, probes_row, top_k, mask=None, **id_rules):
    """(ids int32 [top_k], dists float32 [top_k]) of one query.  d: the handle's distances by LOCAL position."""
    return C.search_row(d, eligible_union(offsets, ids, probes_row, mask, len(d), **id_rules), top_k, **id_rules)


def search(alld, use, offsets, ids, probes, top_k, mask=None, **id_rules):
    return [search_row(alld[u], offsets, ids, probes[q], top_k, mask, **id_rules) for q, u in enumerate(use)]


def table_distances(tables, codes, plain):
    """float32 [nq][n]: every code's distance under every table [M][K], by the handle's rule; -0.0 is read as +0.0."""
    return np.stack([C.distances(np.asarray(t, dtype=np.float32) + np.float32(0), codes, plain) for t in tables])


def search_tables(tables, codes, plain, offsets, ids, probes, top_k, mask=None, **id_rules):
    d = table_distances(tables, codes, plain)
    return search(d, np.arange(len(d)), offsets, ids, probes, top_k, mask, **id_rules)


def search_ip(cb, queries, codes, plain, offsets, ids, probes, top_k, mask=None, **id_rules):
    """(ids int32 [nq][k], scores float32 [nq][k], gaps float32 [nq][k], bias float32 [nq]): dpq_ip_tables, the tables
    form, dpq_ip_scores."""
    _, _, e, B = T.ip_tables(cb, queries)
    rows = search_tables(e, codes, plain, offsets, ids, probes, top_k, mask, **id_rules)
    out_i = np.stack([r[0] for r in rows])
    gaps = np.stack([r[1] for r in rows])
    return out_i, T.ip_scores(B, gaps, out_i), gaps, B


def probe_ip(centroids, queries, nprobe):
    """(lists int32 [nq][nprobe], scores float32 [nq][nprobe]): by (exact score descending, list number)."""
    centroids = np.asarray(centroids, dtype=np.float32)
    return EI.search(centroids, np.asarray(queries, dtype=np.float32).reshape(-1, centroids.shape[1]), nprobe)


def range_row(d, offsets, ids, probes_row, r, mask=None, **id_rules):
    """(ids int32, dists float32) of one query: the eligible nodes of the union with d < r strictly (r = +inf: all of
    them, those at +inf included; r <= 0: none), by (distance bits, id)."""
    id_base, n_local, n_total, even_rule = _rules(len(d), **id_rules)
    u = eligible_union(offsets, ids, probes_row, mask, len(d), **id_rules)        # ascending: position order is id order
    pos = om.positions_of(u, id_base, _renaming_total(n_total, even_rule))
    sel, dd = ne.range_list(np.asarray(d, dtype=np.float32)[pos], np.float32(r))
    return u[sel].astype(np.int32), dd


def range_search(alld, use, offsets, ids, probes, radii, mask=None, **id_rules):
    return [range_row(alld[u], offsets, ids, probes[q], radii[q], mask, **id_rules) for q, u in enumerate(use)]
