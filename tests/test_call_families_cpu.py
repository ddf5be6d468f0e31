"""The families of tests/call_families.py, without a GPU: every entry of the C ABI is placed, and the inputs have the
properties the GPU test (test_call_order_gpu.py) relies on -- from the references and the host routines alone."""
from __future__ import annotations

import numpy as np
import pytest

import call_families as F

FAMILY = pytest.mark.parametrize("family", F.FAMILIES, ids=F.NAMES)


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    _ffi.load_library()
    return _ffi


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_every_symbol_of_the_abi_is_placed(ffi):
    """Reached by a family's run, or left out with a reason -- never both, never neither.  An entry added to one of the
    four ABI tables (_ffi.SYMBOLS, _xabi.XSYMBOLS, _iabi.ISYMBOLS, _babi.BSYMBOLS) fails here, by name, until someone
    places it; so does a family taken out of the matrix."""
    from mcmc_ref_hip import _babi, _iabi, _xabi
    tables = (ffi.SYMBOLS, _xabi.XSYMBOLS, _iabi.ISYMBOLS, _babi.BSYMBOLS)
    assert [len(t) for t in tables] == [143, 10, 11, 17]
    abi = set().union(*tables)
    assert len(abi) == 181                                    # no name in two tables
    reached = {s: f.name for f in F.FAMILIES for s in f.symbols}
    left_out = {s: reason for reason, symbols in F.NOT_IN_THE_MATRIX.items() for s in symbols}
    assert all(reason.strip() for reason in F.NOT_IN_THE_MATRIX)
    assert sum(len(v) for v in F.NOT_IN_THE_MATRIX.values()) == len(left_out), "a symbol is left out twice"
    unknown = sorted((set(reached) | set(left_out)) - abi)
    assert not unknown, f"in none of the four ABI tables: {unknown}"
    both = sorted(set(reached) & set(left_out))
    assert not both, f"reached by a family and left out: {both}"
    unplaced = sorted(abi - set(reached) - set(left_out))
    assert not unplaced, f"neither reached by a family of call_families.FAMILIES nor in NOT_IN_THE_MATRIX: {unplaced}"
    assert len(set(reached) | set(left_out)) == 181
    assert {s for s in abi if s.endswith("_host")} <= set(F.NOT_IN_THE_MATRIX["a host routine"])
    assert reached["mcr_covariance_dev"] == "mean_shift_test"


def test_the_twenty_nine_families_and_their_refusals():
    assert len(F.FAMILIES) == 29 == len(set(F.NAMES)) and [f.index for f in F.FAMILIES] == list(range(29))
    assert F.NAMES[24:] == ["linalg", "gaussian_check", "indicator_ess", "batch_means", "mean_shift_test"]
    assert [f.name for f in F.NEW_FAMILIES] == F.NAMES[24:]
    assert len(F.REFUSED) == 16 == len({r.name for r in F.REFUSED})
    assert {r.family for r in F.REFUSED} <= set(F.NAMES)
    assert all(f.symbols for f in F.FAMILIES)
    assert [r.name for r in F.REFUSED if r.outcome is not None] == ["cholesky_stopped_mid_block"]


# ---- the sizes -------------------------------------------------------------------------------------------------------

def test_small_pooled_lengths_are_odd_distinct_and_below_a_tile():
    small = {f.name: f.pooled("small") for f in F.FAMILIES if f.pooled("small") is not None}
    assert len(small) == 13                                   # every family on a draw tensor or on pooled samples
    assert all(1000 <= m < F.TILE and m % 2 == 1 for m in small.values()), small
    assert len(set(small.values())) == len(small), small


def test_large_pooled_lengths_of_the_sorting_families_carry_32_bit_positions():
    sorting = [f for f in F.FAMILIES if f.sorts]
    assert {f.name for f in sorting} == {"summarize", "enqueue", "diagnose_chains", "two_sample", "sliced_two_sample", "nested_rhat",
                                         "pareto_khat", "psis", "hdi", "weighted_summary"}
    for f in sorting:
        assert f.pooled("small") < F.TILE and f.pooled("large") >= F.WIDE + 1, f.name


def shapes_of(inputs) -> list:
    return [v.shape for v in inputs.values() if isinstance(v, np.ndarray)]


def per_parameter(family, size: str) -> int:
    x = family.inputs(size)["x"]
    return x.size if x.ndim == 1 else x.size // (x.shape[-1] if family.name == "enqueue" else x.shape[0])


@FAMILY
def test_inputs_have_the_declared_shapes_and_seeds(family):
    for size in F.SIZES:
        a, b = family.inputs(size), family.build(size)
        assert a is family.inputs(size)                       # built once
        for k, v in a.items():                                # and the same from the seed again
            if isinstance(v, np.ndarray):
                assert v.tobytes() == b[k].tobytes(), (family.name, size, k)
    m = family.pooled("small")
    if m is not None and "x" in family.inputs("small"):
        assert per_parameter(family, "small") == m, (family.name, m)
    if family.sorts and "x" in family.inputs("large"):
        assert per_parameter(family, "large") == family.pooled("large"), family.name
    assert family.seed("small") != family.seed("large")
    assert len({f.seed(s) for f in F.FAMILIES for s in F.SIZES}) == 2 * len(F.FAMILIES)


def test_special_small_sizes():
    e, s = F.BY_NAME["energy_distance"].inputs("small"), F.BY_NAME["sbc_ranks"].inputs("small")
    assert e["ref"].shape == (3, 130) and e["act"].shape == (3, 70)
    assert s["x"].shape == (3, 2, 129) and s["x4"].shape == (3, 3, 43, 2)
    i = F.ingest()
    assert all(len(t) < 1000 for t in i.f["chain_csv", "small"]["texts"]) and len(i.f["json", "small"]["text"]) < 1000
    assert len(i.f["table_csv", "small"]["data"]) < 1000 and len(F.BY_NAME["read_columns"].inputs("small")["img"]) < 1000
    import test_csv_table_gpu as TT
    import test_json_gpu as TJ
    ints = TJ.expected_from_text(i.f["json", "small"]["text"])[2]             # an all-integer column beside a real one, in both
    assert any(ints) and not all(ints), ints
    table = TT.read_host(i.f["table_csv", "small"]["data"])
    kinds = {str(table.schema.field(n).type) for n in table.column_names if n not in ("chain", "draw")}
    assert kinds == {"int64", "double"}, kinds
    # (the two small draws files of Ingest hold 32 and 20 rows in 1.4 and 1.8 KB: pyarrow's footer for three and four columns)
    assert all(p.stat().st_size < 2048 for p in i.f["files", "small"]["paths"])
    e, s = F.BY_NAME["energy_distance"].inputs("large"), F.BY_NAME["sbc_ranks"].inputs("large")
    assert e["ref"].shape == (9, 300) and e["act"].shape == (9, 260) and s["x"].shape == (9, 7, 2049)
    assert F.BY_NAME["covariance"].inputs("large")["x"].shape == (40, 16385)


def test_sizes_of_the_extension_and_companion_families():
    """Every size sits where it was chosen to: the block size of the factorisation, the LDS limit of the lag kernel, the
    routes and the block of the batch means, the ends of e2e_case's range."""
    from mcmc_ref_hip import _babi, _iabi, _xabi
    from test_batchmeans_refs_cpu import E2E_P
    B, NB = F.BY_NAME, _xabi.MCRX_CHOL_NB
    i = {s: B["linalg"].inputs(s) for s in F.SIZES}
    assert [(i[s]["A"].shape, i[s]["B"].shape) for s in F.SIZES] == [((17, 17), (17, 1)), ((3 * NB + 1,) * 2, (3 * NB + 1, 65))]
    assert all(np.array_equal(i[s]["A"], i[s]["A"].T) and (np.diag(i[s]["A"]) == 1.0).all() for s in F.SIZES)
    i = {s: B["gaussian_check"].inputs(s) for s in F.SIZES}
    assert [(i[s]["ref"].shape, i[s]["act"].shape) for s in F.SIZES] == [((3, 131), (3, 77)), ((2 * NB + 1, 2049), (2 * NB + 1, 1025))]
    for s in F.SIZES:                                         # one parameter dropped: P_live < P; and the gate's condition
        want = B["gaussian_check"].reference(i[s])
        assert int((i[s]["scale"] == 0).sum()) == 1 and (i[s]["scale"] >= 0).all() and want["p_live"] == len(i[s]["scale"]) - 1
        assert np.linalg.cond(want["C_ref"]) <= 2e3 and np.linalg.cond(want["C_act"]) <= 2e3, s
    f = B["indicator_ess"]
    assert f.LDS_WORDS == _iabi.MCI_LDS_WORDS and f.shape("small") == (2, 129, 3, "pcn")
    C_, N, P, layout = f.shape("large")
    assert (C_, P, layout) == (3, 2, "cnp") and N <= _iabi.MCI_MAX_DRAWS
    words = lambda n: C_ * ((n + 63) // 64 + 1)  # noqa: E731
    assert words(N) > _iabi.MCI_LDS_WORDS >= words(N - 1)     # the smallest N on the global route
    assert 2 * (129 // 64 + 2) <= _iabi.MCI_LDS_WORDS         # and the small size on the LDS route
    for s in F.SIZES:
        i = f.inputs(s)
        C_, N, P, layout = f.shape(s)
        x = np.transpose(i["x"], [layout.index(a) for a in "pcn"])
        assert x.shape == (P, C_, N) and i["upper"].shape == (P, 3) and i["x"].flags.c_contiguous
        assert np.array_equal(x[0], np.round(x[0] * 2) / 2) and not np.array_equal(x[1], np.round(x[1] * 2) / 2)
        assert np.array_equal(i["upper"], np.quantile(x.reshape(P, -1), f.PROBS, axis=1).T)
        assert (x[0] == i["upper"][0, 1]).any()               # draws equal to a threshold
    f = B["batch_means"]
    assert f.SHAPES["small"] == (2, 131, 3, 9, "pcn")
    C_, N, P, b, layout = f.SHAPES["large"]
    assert (C_, P, layout) == (3, 130, "cnp") and N == 3 * b + 7 and b % 3 == 0 and _babi.MCB_BLOCK < b < 2 * _babi.MCB_BLOCK and P % 64
    for s in F.SIZES:
        C_, N, P, b, layout = f.SHAPES[s]
        i = f.inputs(s)
        assert i["x"].shape == tuple({"p": P, "c": C_, "n": N}[a] for a in layout) and i["x"].flags.c_contiguous and i["b"] == b
    f = B["mean_shift_test"]
    assert (f.p_live("small"), f.p_live("large")) == (min(E2E_P), max(E2E_P)) == (1, 129)
    assert f.inputs("small")["ref"].shape == (1, 3, 2004) and f.inputs("large")["act"].shape == (130, 4, 3003)
    assert int((f.inputs("large")["scale"] == 0).sum()) == 1


@pytest.mark.parametrize("family", F.NEW_FAMILIES, ids=[f.name for f in F.NEW_FAMILIES])
def test_host_definitions_pass_the_check_at_both_sizes(family, ffi):
    """The family's `check` on what the definitions on the host give: at the chosen sizes the reference alone stays inside
    its gate, so a failure of the GPU test is the device's."""
    for size in F.SIZES:
        i = family.inputs(size)
        got = family.host(i)
        assert isinstance(got, dict) and got == family.host(i)                 # and the host is deterministic, in bits
        family.check(i, got)
    if family.name == "indicator_ess":                        # the large walk ends in the first lag block, and it is a walk
        from mcmc_ref_hip import _iabi
        t = F.unpack(family.host(family.inputs("large")))["trunc"]
        assert (0 < t).all() and (t < _iabi.MCI_LAG_BLOCK).all(), t


@FAMILY
def test_large_values_are_no_plausible_small_values(family):
    """Where the statistic allows an offset: every large draw lies far outside the range of the small draws."""
    if family.name in ("pareto_khat", "psis", "read_columns", "summarize_files", "csv_decode", "json_decode", "csv_table_decode",
                       "write_parquet", "write_csv", "chain_layout", "linalg", "gaussian_check", "indicator_ess", "mean_shift_test"):
        # no offset: the tail fits are about the draws' own scale; files; a matrix; statistics of centred draws or of an
        # indicator at the draws' own quantiles, which a translation leaves where they are (e2e_case's draws are shared)
        return
    assert family.offset("large") == 1000.0 * (family.index + 1) and family.offset("small") == 0.0
    key = {"compare": "ref", "two_sample": "ref", "sliced_two_sample": "ref", "energy_distance": "ref"}.get(family.name, "x")
    small, large = family.inputs("small")[key], family.inputs("large")[key]
    if family.name == "compare":
        small, large = small[np.abs(small) < 100], large[np.abs(large) > 0][:: 7]
        assert np.median(large) > 900.0
        return
    if family.name == "weighted_summary":
        small, large = small[0], large[0]
    if family.name == "sbc_ranks":                            # (edge_sample keeps its second parameter at 1e8 at either size)
        small, large = small[:, 0], large[:, 0]
    assert float(np.min(large)) > float(np.max(np.abs(small))) + 100.0, (family.name, np.min(large), np.max(np.abs(small)))


# ---- the refusals ----------------------------------------------------------------------------------------------------

def arrays_of(inputs) -> list:
    return [v for v in inputs.values() if isinstance(v, np.ndarray)]


@pytest.mark.parametrize("refusal", F.REFUSED, ids=[r.name for r in F.REFUSED])
def test_each_refused_input_has_exactly_its_defect(refusal, ffi):
    i = refusal.inputs()
    arrs = arrays_of(i)
    bad = sum(int((~np.isfinite(a)).sum()) for a in arrs)
    if refusal.outcome is None:
        assert refusal.code() < 0 and refusal.fragment
    else:
        assert refusal.code() == ffi.MCR_OK
    if refusal.defect == "negative_pivot":
        from mcmc_ref_hip import _xabi, gaussian
        NB = _xabi.MCRX_CHOL_NB
        A = i["A"]
        assert bad == 0 and A.shape == (2 * NB + 5,) * 2 and i["info"] == NB + 2
        assert np.array_equal(A - np.diag(np.diag(A)), np.zeros_like(A)) and np.flatnonzero(np.diag(A) != 1.0).tolist() == [NB + 1]
        _, info, logdet = gaussian.cholesky_host(A)              # the definition stops there, with MCR_OK
        assert refusal.outcome((info, logdet, i["info"])) and not refusal.outcome((0, logdet, i["info"]))
        assert not refusal.outcome((info, 0.0, i["info"]))
    elif refusal.defect == "gaussian_limit":
        from mcmc_ref_hip import gaussian
        assert bad == 0 and i["ref"].shape == (129, 2000) and i["act"].shape == (129, 1500)
        r = gaussian.gaussian_check_host(i["ref"], i["act"], i["scale"])     # nothing but the limit is in the way
        assert (r["p_live"], r["info_ref"], r["info_act"]) == (129, 0, 0)
    elif refusal.defect == "companion_limit":
        assert bad == 0 and F.TINY_LIMIT < 256 and F.COMPANION_LIMIT == 1 << 30
        x, b = i["x"], i["batch"]
        if b is None:
            from mcmc_ref_hip import indicator
            assert refusal.family == "indicator_ess" and (indicator.indicator_ess_host(x, -np.inf, 0.0)["ones"] > 0).all()
        else:
            from mcmc_ref_hip import batchmeans
            assert refusal.family == "batch_means" and np.isfinite(batchmeans.batch_means_host(x, batch=b, r=3)["bm"]).all()
    elif refusal.defect == "batch_over_n":
        assert bad == 0 and i["batch"] == i["x"].shape[2] + 1
    elif refusal.defect == "one_nan":
        assert bad == 1 == sum(int(np.isnan(a).sum()) for a in arrs)
    elif refusal.defect == "one_inf":
        assert bad == 1 == sum(int(np.isinf(a).sum()) for a in arrs)
    elif refusal.defect == "three_nonfinite":
        assert bad == 3 and np.isfinite(i["t"]).all()
    elif refusal.defect == "one_negative_weight":
        assert bad == 0 and int((i["w"] < 0).sum()) == 1 and (np.delete(i["w"], np.flatnonzero(i["w"] < 0)) >= 0).all()
    elif refusal.defect == "overflow":
        assert bad == 0
        with np.errstate(over="ignore"):
            d2 = ((i["ref"][:, :, None] - i["act"][:, None, :]) ** 2).sum(axis=0)
        r, a = (int(np.argmax(np.abs(i[k]).max(axis=0))) for k in ("ref", "act"))       # the two huge draws
        assert np.isinf(d2[r, a]) and np.isfinite(np.delete(np.delete(d2, r, axis=0), a, axis=1)).all()
        with pytest.raises(ffi.McrError) as e:
            ffi.energy_distance_host(i["ref"], i["act"])
        assert e.value.code == refusal.code()
    elif refusal.defect == "snappy_preamble":
        diff = [k for k, (a, b) in enumerate(zip(i["good"], i["img"])) if a != b]
        assert diff == [i["at"]] and len(i["good"]) == len(i["img"])
    else:
        assert refusal.defect == "limit" and bad == 0
        x = i["x"]
        assert x[0].size * 8 > F.LOW_LIMIT                    # a parameter's keys alone
    if refusal.name == "summarize_nan_in_last_tile":
        x = i["x"]
        p, c, n = (int(v[0]) for v in np.nonzero(np.isnan(x)))
        M = x.shape[1] * x.shape[2]
        assert M > F.TILE and c * x.shape[2] + n >= (M - 1) // F.TILE * F.TILE       # in time order it lies in the last tile
        assert np.sort(x[p].reshape(-1))[-1] != np.sort(x[p].reshape(-1))[-1]        # and in the sorted order: NaN sorts last


# ---- the host routines accept every input of the matrix ------------------------------------------------------------------

def test_host_routines_accept_every_input(ffi):
    for f in F.FAMILIES:
        for size in F.SIZES:
            for a in arrays_of(f.inputs(size)):
                if a.dtype.kind == "f" and f.name not in ("read_columns", "write_parquet", "write_csv", "compare"):
                    assert np.isfinite(a).all() or f.name == "weighted_summary", (f.name, size)
    B = F.BY_NAME
    for size in F.SIZES:
        i = B["energy_distance"].inputs(size)
        assert np.isfinite(list(ffi.energy_distance_host(i["ref"], i["act"], i["scale"]).values())).all()
        i = B["sbc_ranks"].inputs(size)
        assert ffi.sbc_ranks_host(i["x"], i["t"])["n_draws"] == i["x"].shape[2]
        i = B["autocorr"].inputs(size)
        assert np.isfinite(B["autocorr"].host(i, 0)["tau_pooled"]).all()
        i = B["hdi"].inputs(size)
        assert (ffi.hdi_sorted_host(np.sort(i["x"][0]), B["hdi"].PROBS)[2] >= 0).all()
        i = B["pareto_khat"].inputs(size)
        assert ffi.pareto_fit_host(np.sort(i["x"][0]))[2] > 0
        i = B["psis"].inputs(size)
        assert ffi.psis_host(i["x"][0])["ndraws_tail"] > 0
        i = B["weighted_summary"].inputs(size)
        assert np.isfinite(ffi.weighted_host(i["x"][0], log_weights=i["lw"], quantiles=i["qs"])["mean"])


# ---- margins: a decision of the device must not hang on the last bit of a host sum ------------------------------------------

@pytest.mark.parametrize("size", F.SIZES)
def test_weighted_quantile_thresholds_keep_their_margin(size):
    from test_weighted_refs_cpu import threshold_margin
    f = F.BY_NAME["weighted_summary"]
    i = f.inputs(size)
    wh = f.host_weights(i)
    for p in range(2):                                        # (as test_weighted_gpu.test_log_weights: the inner probabilities)
        assert threshold_margin(i["x"][p], wh, i["qs"][2:5]) >= 1e-9, (size, p)


@pytest.mark.parametrize("size", F.SIZES)
def test_psis_reference_agrees_with_itself(size):
    from test_psis_refs_cpu import assert_reference_agrees, check
    from mcmc_ref_hip import _ffi
    for p, row in enumerate(F.BY_NAME["psis"].inputs(size)["x"]):
        ref = assert_reference_agrees(row, (size, p))
        host = _ffi.psis_host(row)
        check({k: host[k] for k in ("khat", "ndraws_tail", "log_weights")}, ref, ("host", size, p))


@pytest.mark.parametrize("size", F.SIZES)
def test_autocorrelation_windows_keep_their_margin(size):
    from test_acf_refs_cpu import gate, one
    f = F.BY_NAME["autocorr"]
    i = f.inputs(size)
    for p in range(i["x"].shape[0]):
        gate(one(f.host(i, p), 0), i["x"][p], i["L"], False, 5.0, (size, p))       # asserts the reference's margin first
