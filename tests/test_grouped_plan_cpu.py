"""The grouped Schur build's plan (csrc/grouped_plan.h through HMiGroupedPlanQuery, api.grouped_plan): eligibility, the job
list and the contributor lists of the ordered scatter, on hand-made operators.  Host arithmetic only: no GPU."""
import numpy as np

JOB_ROWS = 8          # csrc/grouped_plan.h: HDM_GROUPED_JOB_ROWS


def _plan(m, cones):
    from hdsdp_amd import api
    return api.grouped_plan(m, cones)


def _truss1_shape():
    """six blocks of dimension 2 and one of dimension 1 over m = 6 rows (truss1's shape)"""
    m = 6
    cones = [(2, sorted({k, (k + 1) % m, (k + 3) % m})) for k in range(6)] + [(1, list(range(m)))]
    return m, cones


def _chain(nblocks=5, per=5, n=9):
    """blocks with disjoint rows"""
    return nblocks * per, [(n, list(range(k * per, (k + 1) * per))) for k in range(nblocks)]


def _arrow(nblocks=6, own=4, link=3, n=10):
    """every block has rows of its own and shares the `link` last rows of the operator"""
    m = nblocks * own + link
    return m, [(n, list(range(k * own, (k + 1) * own)) + list(range(m - link, m))) for k in range(nblocks)]


def _numpy_contributors(cones):
    """the definition: (col, row) of M's lower triangle -> [(slot, packed local index)], slots in the order of the cones;
    row -> [(slot, local row)]"""
    dm, dv = {}, {}
    for s, (_, rows) in enumerate(cones):
        ml = len(rows)
        for q in range(ml):
            dv.setdefault(rows[q], []).append((s, q))
            for p in range(q, ml):
                key = (min(rows[p], rows[q]), max(rows[p], rows[q]))
                dm.setdefault(key, []).append((s, q * ml - q * (q - 1) // 2 + (p - q)))
    return dm, dv


def _check_lists(m, cones):
    p = _plan(m, cones)
    assert p["cones"] == len(cones) and list(p["slot_of"]) == list(range(len(cones)))
    dm, dv = _numpy_contributors(cones)
    keys = sorted(dm)
    assert [(int(c), int(r)) for c, r in zip(p["m_col"], p["m_row"])] == keys
    assert np.all(p["m_row"] >= p["m_col"])
    for e, key in enumerate(keys):
        lo, hi = int(p["m_ptr"][e]), int(p["m_ptr"][e + 1])
        assert list(zip(p["m_slot"][lo:hi].tolist(), p["m_idx"][lo:hi].tolist())) == dm[key]
        assert np.all(np.diff(p["m_slot"][lo:hi]) > 0)                       # ascending cone order
    rows = sorted(dv)
    assert p["v_row"].tolist() == rows
    for e, r in enumerate(rows):
        lo, hi = int(p["v_ptr"][e]), int(p["v_ptr"][e + 1])
        assert list(zip(p["v_slot"][lo:hi].tolist(), p["v_idx"][lo:hi].tolist())) == dv[r]
        assert np.all(np.diff(p["v_slot"][lo:hi]) > 0)
    assert int(p["m_ptr"][-1]) == sum(len(r) * (len(r) + 1) // 2 for _, r in cones)
    return p


def test_contributor_lists_equal_the_definition_in_ascending_cone_order():
    for m, cones in (_truss1_shape(), _chain(), _arrow()):
        _check_lists(m, cones)
    # the arrow's linking rows: every block contributes to each of their entries, a chain's entries have one contributor each
    m, cones = _arrow()
    p = _plan(m, cones)
    last = int(np.flatnonzero((p["m_row"] == m - 1) & (p["m_col"] == m - 1))[0])
    assert int(p["m_ptr"][last + 1] - p["m_ptr"][last]) == len(cones)
    m, cones = _chain()
    assert np.all(np.diff(_plan(m, cones)["m_ptr"]) == 1)


def test_rows_in_another_local_order_land_on_the_lower_triangle():
    """a cone whose local order is not ascending (direct rows come last): destinations are still (row >= col)"""
    m, cones = 7, [(4, [5, 1, 6, 0]), (4, [2, 6, 3])]
    _check_lists(m, cones)


def test_every_owned_row_is_in_exactly_one_job_and_a_cone_without_rows_has_one():
    m = 130
    cones = [(8, list(range(40))), (8, list(range(40, 80))), (8, list(range(80, 120))), (5, []), (3, [121, 7, 129])]
    p = _plan(m, cones)
    assert p["cones"] == 5
    jobs = p["jobs"]
    assert len(jobs) == 3 * 5 + 1 + 1 and len(jobs) > 3      # three blocks of forty rows fill more than three workgroups
    for s, (_, rows) in enumerate(cones):
        mine = jobs[jobs[:, 0] == s]
        assert int(mine[:, 3].sum()) == 1 and mine[0, 3] == 1 and mine[0, 1] == 0     # one first job: the scalars
        covered = np.concatenate([np.arange(q0, q1) for _, q0, q1, _ in mine] + [np.zeros(0, dtype=int)])
        assert sorted(covered.tolist()) == list(range(len(rows)))
        assert np.all(mine[:, 2] - mine[:, 1] <= JOB_ROWS)
    empty = jobs[jobs[:, 0] == 3]
    assert len(empty) == 1 and empty[0, 1] == empty[0, 2] == 0 and empty[0, 3] == 1


def test_eligibility_at_the_dimension_and_data_bounds():
    small = (8, [0, 1])
    for n, ok in ((64, True), (65, False), (1, True), (128, False)):
        p = _plan(4, [small, (n, [2, 3]), small])
        assert bool(p["eligible"][1]) == ok and p["cones"] == (3 if ok else 2) and int(p["slot_of"][1]) == (1 if ok else -1)
        assert int(p["slot_of"][2]) == (2 if ok else 1)
    # mloc * n16 * n16 <= 2^19: 128 rows at n16 = 64, 2048 at n16 = 16 (n = 17 has n16 = 32: 512)
    for n, rows, ok in ((64, 128, True), (64, 129, False), (49, 129, False), (16, 2048, True), (16, 2049, False), (17, 512, True),
                        (17, 513, False)):
        p = _plan(rows + 2, [small, (n, list(range(2, rows + 2)))])
        assert bool(p["eligible"][1]) == ok, (n, rows)
        assert p["cones"] == (2 if ok else 0) and p["n_eligible"] == (2 if ok else 1)
    # a cone of another kind (LP, device group, host cone, synthetic, streamed) is never grouped
    p = _plan(4, [small, (8, [2, 3], False), small])
    assert p["eligible"].tolist() == [True, False, True] and p["slot_of"].tolist() == [0, -1, 1]


def test_fewer_than_two_eligible_cones_leave_the_pass_unused():
    p = _plan(4, [(8, [0, 1]), (65, [2, 3])])
    assert p["cones"] == 0 and p["n_eligible"] == 1 and len(p["jobs"]) == 0 and len(p["m_row"]) == 0 and len(p["v_row"]) == 0
    assert p["slot_of"].tolist() == [-1, -1] and p["staging_doubles"] == 0
    p = _plan(3, [])
    assert p["cones"] == 0


def test_staging_memory_is_what_the_design_says():
    """X (n16^2), the packed local Gram (mloc (mloc + 1) / 2, at least one word) and 3 mloc + 4 doubles per grouped cone"""
    cones = [(9, [0, 1, 2]), (40, [1, 3]), (5, [])]
    p = _plan(4, cones)
    want = sum(((n + 15) // 16 * 16) ** 2 + max(1, len(r) * (len(r) + 1) // 2) + 3 * len(r) + 4 for n, r in cones)
    assert p["staging_doubles"] == want


def test_bad_arguments_are_refused():
    import pytest
    from hdsdp_amd import api
    with pytest.raises(api.HDSDPError):
        _plan(3, [(4, [0, 3])])           # a row outside the operator
