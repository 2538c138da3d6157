"""Host-side parts of gpitch_amd.predict_many (no device): the scope refusals, the (latent GP, frame tile) work list and
output offsets of one gp_pdgpb_predict call, and the split of a call's frames into launches."""
import numpy as np
import pytest

from helpers import pdgp_from_problem


def _model(**kw):
    from gpitch_amd.synth import make_problem
    return pdgp_from_problem(make_problem(600, 16, 2, num_partials=3, seed=3), **kw)


def test_accepts_the_scope_without_a_minibatch_limit():
    """a model trained with minibatch_size = 5000 (above optimize_many's 1024) is predictable: prediction does not
    use the minibatch"""
    from gpitch_amd.pdgp_batch import check_batchable, check_predictable
    from gpitch_amd.synth import make_problem
    big = pdgp_from_problem(make_problem(6000, 16, 1, num_partials=2, seed=4), minibatch_size=5000)
    ms = [_model(), _model(minibatch_size=100), big]
    xs = [np.linspace(0., 0.01, 7), np.zeros((0, 1)), np.linspace(0., 0.02, 3).reshape(-1, 1)]
    got, gx = check_predictable(ms, xs)
    assert got == ms
    assert [x.shape for x in gx] == [(7,), (0,), (3,)] and all(x.dtype == np.float64 for x in gx)
    got, gx = check_predictable(ms, np.arange(5, dtype=np.float32).reshape(-1, 1))       # one array for every model
    assert len(gx) == 3 and all(x.dtype == np.float64 and x.shape == (5,) for x in gx)
    with pytest.raises(ValueError):
        check_batchable([big])


@pytest.mark.parametrize("what", ["whiten", "float32", "pair", "shard", "M", "partials", "kernel_m12sm",
                                  "kernel_prod", "duplicate", "empty", "not_a_model", "xnews_length", "xnew_shape"])
def test_refusals_name_the_single_model_path(what):
    from gpitch_amd.pdgp_batch import check_predictable, predict_many
    from gpitch_amd.synth import make_problem
    xnews, models, err = None, None, NotImplementedError
    if what == "whiten":
        models = [_model(whiten=False)]
    elif what == "float32":
        models = [_model(float_type=np.float32)]
    elif what == "pair":
        models = [_model(float_type=(np.float64, np.float32))]
    elif what == "shard":
        models = [_model(shard=(0, 2))]
    elif what == "M":
        models, err = [pdgp_from_problem(make_problem(600, 129, 1, num_partials=2))], ValueError
    elif what == "partials":
        models, err = [pdgp_from_problem(make_problem(600, 16, 1, num_partials=33))], ValueError
    elif what == "kernel_m12sm":
        p = make_problem(600, 16, 1, num_partials=2)
        p["kern_com"][0]["type"] = "matern12sm"
        models = [pdgp_from_problem(p)]
    elif what == "kernel_prod":
        p = make_problem(600, 16, 1, num_partials=2)
        p["kern_com"][0]["type"] = "mercer_matern52sm"
        models = [pdgp_from_problem(p)]
    elif what == "duplicate":
        m = _model()
        models, err = [m, m], ValueError
    elif what == "empty":
        models, err, xnews = [], ValueError, []
    elif what == "not_a_model":
        models, err = [_model(), object()], ValueError
    elif what == "xnews_length":
        models, err, xnews = [_model(), _model()], ValueError, [np.zeros(3)]
    else:
        models, err, xnews = [_model()], ValueError, [np.zeros((4, 2))]
    if xnews is None:
        xnews = [np.linspace(0., 0.01, 5) for _ in models]
    with pytest.raises(err) as e:
        check_predictable(models, xnews)
    if what not in ("duplicate", "empty", "not_a_model", "xnews_length", "xnew_shape"):
        assert "Pdgp.predict_act_n_com" in str(e.value)
    with pytest.raises(err):           # refused by the public entry before any device work (no GPU here)
        predict_many(models, xnews)


def test_work_list_and_offsets_of_ragged_inputs():
    """frame counts 0, 1, T - 1, T, T + 1 and a long one over models with P = 1, 3, 2, 1, 1, 2"""
    from gpitch_amd.pdgp_batch import PREDICT_TILE as T, predict_layout
    P = [1, 3, 2, 1, 1, 2]
    n = [0, 1, T - 1, T, T + 1, 10 * T + 5]
    lay = predict_layout(P, n)
    per_gp_tiles = []
    for Pk, nk in zip(P, n):
        per_gp_tiles += [-(-nk // T)] * (2 * Pk)
    np.testing.assert_array_equal(per_gp_tiles, [0] * 2 + [1] * 6 + [1] * 4 + [1] * 2 + [2] * 2 + [11] * 4)
    np.testing.assert_array_equal(lay["tile_start"], np.concatenate([[0], np.cumsum(per_gp_tiles)]))
    assert lay["tile_start"].dtype == np.int64 and lay["tile_start"][-1] == 6 + 4 + 2 + 4 + 44
    np.testing.assert_array_equal(lay["x_off"], [0, 0, 1, T, 2 * T, 3 * T + 1, 13 * T + 6])
    np.testing.assert_array_equal(lay["out_base"], np.concatenate([[0], np.cumsum(2 * np.array(P) * n)]))
    np.testing.assert_array_equal(lay["src_base"], np.concatenate([[0], np.cumsum(np.array(P) * n)]))
    # each latent GP's row inside its model's block: rows [g_0..g_{P-1}, f_0..f_{P-1}] of n_k frames
    g = 0
    for k, (Pk, nk) in enumerate(zip(P, n)):
        for r in range(2 * Pk):
            assert lay["gp_out"][g] == lay["out_base"][k] + r * nk
            assert lay["gp_src"][g] == (lay["src_base"][k] + r * nk if r < Pk else -1)
            g += 1
    assert g == len(lay["gp_out"]) == len(lay["tile_start"]) - 1


def test_offsets_stay_64_bit_past_2_to_the_31():
    from gpitch_amd.pdgp_batch import predict_layout
    n = [1 << 28, 1 << 28, 5]
    lay = predict_layout([3, 2, 1], n)
    assert lay["out_base"][-1] == 2 * (3 + 2) * (1 << 28) + 10 > 2 ** 31
    assert lay["gp_out"][-1] == lay["out_base"][2] + 5


@pytest.mark.parametrize("limit", [6, 64, 100, 1 << 22])
def test_chunks_cover_every_frame_once_within_the_limit(limit):
    from gpitch_amd.pdgp_batch import predict_chunks
    P = [1, 3, 2, 1]
    n = [0, 70, 1, 129]
    chunks = predict_chunks(P, n, limit)
    seen = [np.zeros(nk, dtype=int) for nk in n]
    for c in chunks:
        assert c.shape == (4, 2) and c.dtype == np.int64
        load = int(np.sum(2 * np.array(P) * c[:, 1]))
        assert 0 < load <= max(limit, 2 * max(P))
        for k, (s, m) in enumerate(c):
            seen[k][s:s + m] += 1
    assert all(np.all(s == 1) for s in seen)
    if limit >= 2 * sum(np.array(P) * n):
        assert len(chunks) == 1


def test_chunks_of_a_call_without_frames():
    from gpitch_amd.pdgp_batch import predict_chunks
    chunks = predict_chunks([1, 2], [0, 0])
    assert len(chunks) == 1 and not chunks[0][:, 1].any()
