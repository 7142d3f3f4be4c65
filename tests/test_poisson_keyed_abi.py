"""CPU suite (no GPU touched): the C entry point of the keyed Poisson select and the Python keywords above it
(DESIGN.md section 21)."""
import ctypes as C

import pytest


def _lib():
    from bliss_gnn_amd import _lib
    return _lib


def test_symbol_and_einval_before_any_launch():
    lib = _lib()
    fn = lib.lib.bliss_poisson_select_keyed
    assert "bliss_poisson_select_keyed" in lib.SIGNATURES and fn.restype is C.c_int
    ws, step = lib.LayerWs(), C.c_int64(0)                        # never dereferenced: every case returns before a launch
    sp = C.addressof(step)
    assert fn(None, 4, 0.9999, 1, sp, 0, 1, 16, None) == lib.EINVAL
    assert fn(C.byref(ws), 4, 0.9999, 1, None, 0, 1, 16, None) == lib.EINVAL
    assert fn(C.byref(ws), -1, 0.9999, 1, sp, 0, 1, 16, None) == lib.EINVAL
    for layer in (-1, 256, 1 << 20):
        assert fn(C.byref(ws), 4, 0.9999, 1, sp, layer, 0, 16, None) == lib.EINVAL
    assert step.value == 0


def test_header_declares_the_entry_point():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bliss_gnn.h")).read()
    assert "int bliss_poisson_select_keyed(const bliss_layer_ws_t* ws, int32_t fanout, double eps, uint64_t seed, int64_t* step_dev," in text


def test_class_keywords():
    import bliss_gnn_amd as bg
    for cls in (bg.PoissonBanditLadiesSampler, bg.PoissonLadiesSampler):
        s = cls([4, 4])
        assert s.draw == "host" and s.layer_dependency is False and s._poisson
        s = cls([4, 4], draw="device")
        assert s.draw == "device" and s.layer_dependency is False and s.draw_step() == 0
        s.reset_draw(seed=9, step=5)
        assert s.draw_step() == 5
        s = cls([4, 4], draw="device", layer_dependency=True)
        assert s.draw == "device" and s.layer_dependency is True
        with pytest.raises(ValueError):
            cls([4, 4], draw="gpu")
        with pytest.raises(ValueError):
            cls([4, 4], layer_dependency=True)
        with pytest.raises(ValueError):
            cls([4, 4], draw="host", layer_dependency=True)
        assert hasattr(s, "check_errors") and hasattr(s, "sample_blocks_static") and hasattr(s, "finish_static")
    assert hasattr(bg.PoissonBanditLadiesSampler([4], draw="device"), "exp3")
    assert bg.PoissonBanditLadiesSampler([4], draw="device").exp3_weights is None
    # the multinomial samplers' keyword is what it was
    assert bg.BanditLadiesSampler([4], draw="device").draw == "device" and bg.LadiesSampler([4]).draw == "host"
    with pytest.raises(ValueError):
        bg.LadiesSampler([4], draw="device", layer_dependency=True)


def test_make_sampler_names():
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    s = fit.make_sampler("poisson-bandit-keyed", [4, 3], importance_sampling=0, eta=0.2, model="gat")
    assert type(s) is bg.PoissonBanditLadiesSampler and s.draw == "device" and s.nodes_per_layer == [4, 3]
    assert s.importance_sampling == 0 and s.eta == 0.2 and s.model == "gat" and s.node_embedding == "features"
    s = fit.make_sampler("poisson-ladies-keyed", [4, 3])
    assert type(s) is bg.PoissonLadiesSampler and s.draw == "device" and s.nodes_per_layer == [4, 3]
    # unchanged: the Poisson names ignore draw= and keep the stream draw
    for name, cls in (("poisson-bandit", bg.PoissonBanditLadiesSampler), ("poisson-ladies", bg.PoissonLadiesSampler)):
        for draw in ("host", "device"):
            s = fit.make_sampler(name, [4], draw=draw)
            assert type(s) is cls and s.draw == "host" and s.layer_dependency is False
