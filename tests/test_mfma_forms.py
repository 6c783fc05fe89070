"""not-gpu: the conditions tests/test_gpu_mfma_forms.py leans on (tests/mfma_forms.py).  Through the plan probe
(tests/host/mfma_plan_probe.cpp, the launchers' own choice): every row runs the instantiations it names, and the rows
together name every instantiation of tests/test_mfma_plan.py's list but those of UNREACHED, which is printed.  From the table
alone: the axes of the issue are present (feature counts at both sides of every wave-count step, the remainders of both tile
widths, the row counts around the staged chunks, the row-chunk cases, a row without bias), the windows are 100 times larger
outside the feature ranges, and the oracle runs every row."""

import numpy as np
import pytest

import mfma_forms as mf
import test_mfma_plan as tp
from mfma_forms import ROW_NAMES, ROWS


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tp.build(tmp_path_factory.mktemp("mfma_forms"), "mfma_plan_probe")

    def launches(name, f32):
        out = []
        for c in mf.calls(name, f32):
            out += tp.parse(tp.run(exe, *c, **ROWS[name]["knobs"]))
        return out
    return launches


def test_the_rows_and_their_names_are_one_list():
    assert set(mf.REACHES) == set(ROW_NAMES) and len(ROW_NAMES) == len(ROWS)
    assert len(set(r["seed"] for r in ROWS.values())) == len(ROWS)
    assert all(set(r["knobs"]) <= set(mf.KNOBS) for r in ROWS.values())
    assert 55 <= len(ROWS) <= 75


@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_row_runs_what_it_names(probe, name):
    ran = set(tp.inst(l) for f32 in (0, 1) for l in probe(name, f32))
    print("%s: %s" % (name, sorted(ran)))
    assert set(mf.REACHES[name]) <= ran, sorted(set(mf.REACHES[name]) - ran)
    assert ran <= tp.INSTANTIATIONS


def test_the_table_names_every_instantiation_but_the_unreached():
    named = set().union(*[set(v) for v in mf.REACHES.values()])
    print("instantiations no row runs: %s" % (list(mf.UNREACHED) or "none"))
    assert not set(mf.UNREACHED) & named and set(mf.UNREACHED) <= tp.INSTANTIATIONS
    for n in sorted(tp.INSTANTIATIONS - named - set(mf.UNREACHED)):
        print("not named by any row:", n)
    assert named | set(mf.UNREACHED) == tp.INSTANTIATIONS
    assert mf.UNREACHED == ()      # every call site shape is reachable: see the module text of mfma_forms.py


def test_fast32_names_only_where_a_row_names_an_f32_instantiation():
    for name in ROW_NAMES:
        assert any("F32=1" in n for n in mf.REACHES[name]), name    # every row runs under both precisions


def _nfun(name, trans):
    r = ROWS[name]
    return (r["ntfe"] if trans else r["nsfe"]) + int(r["bias"])


def test_the_axes_are_present(probe):
    S = [n for n in ROW_NAMES if ROWS[n]["site"] == "S"]
    F = [n for n in ROW_NAMES if ROWS[n]["site"] == "F"]
    W = [n for n in ROW_NAMES if ROWS[n]["site"] == "W"]
    # count NW by nfun, both sides of every step, and the second feature tile
    assert {48, 49, 96, 97, 144, 145, 192, 193, 384, 385} <= set(_nfun(n, False) for n in S)
    assert ROWS["s_nf49"]["nsfe"] == 48      # the bias column alone in the second wave tile
    # feature tail
    assert {1, 3, 4, 5, 31, 32, 33} <= set(ROWS[n]["nsfe"] for n in S) and mf.SFS == 3
    # score forms: N-tiles and 256-row tiles
    assert {8, 24, 40, 56} <= set(ROWS[n]["L"] for n in S)
    assert {1, 255, 256, 257, 513} <= set(mf.n_windows(ROWS[n]["Ts"]) for n in S)
    # narrow remainders (48-wide tiles): MT = 1, 2, 3 and a full tile plus 1
    assert {5, 20, 40, 50} <= set(ROWS[n]["L"] for n in S)
    # 8-wave remainders (64-wide tiles in f64): 81, 100, 121, 196 outputs, under the three knob settings, with and without a row map
    for rows, x in ((F, 1), (W, 0)):
        for knobs in ({}, mf.WS0, mf.WS0_DB0):
            got = set(ROWS[n]["L"] ** 2 for n in rows if ROWS[n]["knobs"] == knobs and _nfun(n, True) >= 193)
            assert {81, 100, 121, 196} <= got, (x, knobs, got)
    l = [x for x in probe("f_ws_121", 0) if x["call"] == "counts" and x["n_out"] == 121]
    assert [(x["kernel"], x["mt"], x["o_base"]) for x in l] == [("ws", 4, 0), ("ws", 4, 64)]     # the MT = 4 remainder at o_base 64
    l = [x for x in probe("f_ws_196", 0) if x["call"] == "counts" and x["n_out"] == 196]
    assert [(x["mt"], x["o_base"], x["gy"], x["gx"]) for x in l] == [(4, 0, 3, 2), (1, 192, 1, 2)]  # three full tiles and MT = 1; two feature tiles
    # split form: 196 outputs (the second workgroup holds 4), 169 stay narrow
    l = [x for x in probe("f_split_15", 0) if x["call"] == "counts" and x["n_out"] == 196]
    assert [(x["kernel"], x["gy"], x["o_step"]) for x in l] == [("split", 2, 192)] and 196 - 192 == 4
    assert all(x["kernel"] == "plain" for x in probe("f_nosplit_169", 0) if x["call"] == "counts")
    # score forms from 192 features on
    sc = lambda n: [(x["kernel"], x["mw"], x["ntw"], x["nt"], x["o_base"], x["gy"]) for x in probe(n, 0) if x["call"] == "scores" and x["n_out"] > 60]
    assert sc("f_ws_100") == [("ws", 2, 7, 0, 0, 1)]
    assert sc("f_ws_121") == [("ws", 4, 3, 0, 0, 1), ("single", 0, 0, 2, 96, 1)]                    # the "no 6a + 7b split" fall-through
    assert sc("f_ws_144") == [("ws", 4, 3, 0, 0, 1), ("single", 0, 0, 3, 96, 1)]
    assert sc("f_ws_196") == [("ws", 4, 3, 0, 0, 1), ("ws", 2, 7, 0, 96, 1)]
    assert ROWS["f_ws_144"]["ntfe"] == 192 and ROWS["f_ws_100_191"]["ntfe"] == 191
    assert all(k == "single" for k, *_ in sc("f_ws_100_191")) and all(k == "single" for k, *_ in sc("f_noscws_121"))
    # rows of the count kernels: KC - 1, KC, KC + 1, 2 KC + 1, 3 KC + 1 per KC, counted over the calls that run that KC
    rows_by_kc = {16: set(), 32: set(), 64: set()}
    for n in ROW_NAMES:
        r = ROWS[n]
        for x in probe(n, 0):
            if x["call"] == "counts":
                trans = x["n_out"] == r["L"] ** 2 and r["site"] != "S"
                rows_by_kc[x["kc"]].add(sum(r["Ts"]) if trans and r["site"] == "F" else mf.n_windows(r["Ts"]))
    for kc, have in rows_by_kc.items():
        assert {kc - 1, kc, kc + 1, 2 * kc + 1, 3 * kc + 1} <= have, (kc, sorted(have))
    # several row chunks
    assert mf.n_windows(ROWS["s_chunks"]["Ts"]) == 4129 > 4096 and 4129 - 4096 == 33 and ROWS["s_chunks"]["L"] == 3
    r = ROWS["f_chunks"]
    assert sum(r["Ts"]) == 200 and r["knobs"] == {"SCRF_TRANS_CHUNKS": "3"} and -(-200 // 3) == 67 and 67 % 32 != 0
    # bias
    assert (mf.STATE_BIAS, mf.TRANS_BIAS) == (0.1, 0.3) and float(np.float32(0.1)) != 0.1 and float(np.float32(0.3)) != 0.3
    assert [n for n in ROW_NAMES if not ROWS[n]["bias"]] == ["s_nobias"]


def test_windows_are_a_hundred_times_larger_outside_the_feature_ranges():
    for name in ("s_tail5", "f_nw2_mt2", "w_split_16"):
        c = mf.FormCase(name)
        X = np.concatenate(c.windows)
        assert X.dtype == np.float32 and X.shape[1] == c.F and not c.inside[:mf.SFS].any() and not c.inside[-3:].any()
        assert np.abs(X[:, c.inside]).max() <= 1.0 and (X[:, c.inside] < 0).any()
        if X.shape[0] >= 16:
            assert (np.abs(X[:, ~c.inside]).max(axis=0) > 50.0).all()
        assert int(c.inside.sum()) == c.row["nsfe"] + c.row["ntfe"]
        o = c.ocfg
        assert o.state_fidx_start == mf.SFS and (c.row["ntfe"] == 0 or o.trans_fidx_start == o.state_fidx_end + 1 + mf.GAP)
        assert c.inside[o.state_fidx_start] and c.inside[o.state_fidx_end] and not c.inside[o.state_fidx_end + 1]


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_oracle_runs_every_row(name):
    c = mf.FormCase(name)
    g, numer, zx = mf.reference(name)
    assert np.isfinite(g).all() and np.isfinite(numer).all() and np.isfinite(zx).all()
    # both blocks carry a gradient, and every weight has an owner the failure text can name
    # (a batch of one-frame utterances has no transition: its transition block is zero, and the GPU test takes the deviation
    # of a zero block as absolute)
    assert np.abs(g[c.is_state]).max() > 0 and (c.is_state.all() or max(c.Ts) == 1 or np.abs(g[~c.is_state]).max() > 0)
    assert [n for n in ROW_NAMES if max(ROWS[n]["Ts"]) == 1] == ["s_tail1"]
    assert c.describe(int(np.argmax(np.abs(g))))
    # at most about 6000 terms of magnitude at most 1 per component (the bound's reasoning in test_gpu_mfma_forms.py)
    assert max(sum(c.Ts), mf.n_windows(c.Ts)) <= 6000
