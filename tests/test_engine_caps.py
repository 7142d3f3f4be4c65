"""The sampler engine's capacity rules (_engine.layer_caps, _engine.static_caps): pure functions of the kind of layer, the graph's
sizes, the seed count and the fanouts.  The expected numbers are worked out by hand from the rules:

  layer-wise   K = min(V, int(1.25 * (f + S)) + 64)          B = min(E, max(2^16, 48 * K))
  neighbor     B = min(E, S * f)  (replace: min(2^31 - 1, S * f))          K = min(V, S + min(B, E))
  LABOR        B = min(E, 2 * S * f + 4096)                   K = min(V, S + B)
  f < 0        B = min(E, max(2^16, 48 * S))                  K = V
  multinomial  K >= min(V, f + S)  (host draw: f + S + 64);  every layer's S >= the previous layer's K
"""
from bliss_gnn_amd._engine import KINDS, layer_caps, static_caps


def _skb(caps):
    assert all(c["C"] == caps[0]["C"] for c in caps)
    return [(c["S"], c["K"], c["B"]) for c in caps]


def test_the_eleven_kinds():
    assert sorted(KINDS) == sorted(["stream", "poisson_keyed", "multinomial_host", "multinomial", "multinomial_replace", "neighbor",
                                    "wneighbor", "neighbor_replace", "labor", "labor_is", "wlabor"])
    assert [k for k in KINDS if KINDS[k].family == "node"] == ["neighbor", "wneighbor", "neighbor_replace", "labor", "labor_is", "wlabor"]
    assert [k for k in KINDS if KINDS[k].split] == ["stream"] and [k for k in KINDS if KINDS[k].torch_rng] == ["stream"]
    assert [k for k in KINDS if not KINDS[k].keyed] == ["stream", "multinomial_host"]


def test_layer_wise_rule():
    for kind in ("stream", "poisson_keyed", "multinomial", "multinomial_replace", "multinomial_host"):
        # 1.25 * 14 = 17.5 -> 17 + 64 = 81; 48 * 81 < 2^16 and 2^16 > |E|: B = |E|.  Then S = 81: int(1.25 * 84) + 64 = 169
        caps = layer_caps(kind, 1000, 5000, 10, [4, 3])
        assert _skb(caps) == [(10, 81, 5000), (81, 169, 5000)] and caps[0]["C"] == 1000
    # 48 * K over 2^16: int(1.25 * 2100) + 64 = 2689, 48 * 2689 = 129072
    assert _skb(layer_caps("stream", 100000, 10 ** 6, 2000, [100])) == [(2000, 2689, 129072)]
    # 2^16 over 48 * K, under |E|
    assert _skb(layer_caps("stream", 100000, 10 ** 6, 10, [4])) == [(10, 81, 65536)]
    # K capped by V: int(1.25 * 1100) + 64 = 1439 > 1000
    assert _skb(layer_caps("poisson_keyed", 1000, 5000, 900, [200])) == [(900, 1000, 5000)]


def test_neighbor_rule():
    for kind in ("neighbor", "wneighbor"):
        # S * f under |E|: B = 40, K = 10 + 40; then B = 150, K = 50 + 150
        assert _skb(layer_caps(kind, 1000, 5000, 10, [4, 3])) == [(10, 50, 40), (50, 200, 150)]
        # S * f over |E| in the second layer: B = 100, K = 50 + 100
        assert _skb(layer_caps(kind, 1000, 100, 10, [4, 3])) == [(10, 50, 40), (50, 150, 100)]
        # K capped by V
        assert _skb(layer_caps(kind, 120, 5000, 10, [4, 3])) == [(10, 50, 40), (50, 120, 150)]
        # a negative fanout: K = V, B = min(E, max(2^16, 480)); then S = 1000: B = 3000, K = min(1000, 4000)
        assert _skb(layer_caps(kind, 1000, 5000, 10, [-1, 3])) == [(10, 1000, 5000), (1000, 1000, 3000)]
        assert _skb(layer_caps(kind, 10 ** 5, 10 ** 6, 10, [-1])) == [(10, 10 ** 5, 65536)]
        assert _skb(layer_caps(kind, 10 ** 5, 10 ** 6, 2000, [-1])) == [(2000, 10 ** 5, 96000)]


def test_neighbor_rule_with_replacement():
    # |E| is no bound on B (a column of fewer than f edges holds f block edges), only on the new sources: K = 50 + min(150, 100)
    assert _skb(layer_caps("neighbor_replace", 1000, 100, 10, [4, 3])) == [(10, 50, 40), (50, 150, 150)]
    # B capped by 2^31 - 1
    assert _skb(layer_caps("neighbor_replace", 2 * 10 ** 9, 100, 10 ** 9, [4])) == [(10 ** 9, 10 ** 9 + 100, 2 ** 31 - 1)]
    # a negative fanout: the rule without replacement
    assert _skb(layer_caps("neighbor_replace", 1000, 5000, 10, [-1, 3])) == [(10, 1000, 5000), (1000, 1000, 3000)]


def test_labor_rule():
    for kind in ("labor", "labor_is", "wlabor"):
        # 2 * 10 * 4 + 4096 = 4176 under |E|, K = min(1000, 4186); then 2 * 1000 * 3 + 4096 over |E|
        assert _skb(layer_caps(kind, 1000, 5000, 10, [4, 3])) == [(10, 1000, 4176), (1000, 1000, 5000)]
        assert _skb(layer_caps(kind, 10 ** 5, 10 ** 6, 10, [4])) == [(10, 4186, 4176)]
        assert _skb(layer_caps(kind, 1000, 5000, 10, [-1, 3])) == [(10, 1000, 5000), (1000, 1000, 5000)]


def test_existing_capacities():
    have = [dict(S=5, C=1000, K=500, B=100, E=77, X=9), dict(S=500, C=1000, K=90, B=6000, E=77, X=9)]
    # more seeds than they hold: merged (max) with the fresh (10, 81, 5000), (81, 169, 5000); the static-only keys go
    caps = layer_caps("stream", 1000, 5000, 10, [4, 3], have)
    assert _skb(caps) == [(10, 500, 5000), (500, 169, 6000)] and all(sorted(c) == ["B", "C", "K", "S"] for c in caps)
    assert _skb(layer_caps("neighbor", 1000, 5000, 10, [4, 3], have)) == [(10, 500, 100), (500, 200, 6000)]
    assert have[0] == dict(S=5, C=1000, K=500, B=100, E=77, X=9)                # (pure)
    # they hold the seeds: kept as they are, the same object
    assert layer_caps("stream", 1000, 5000, 5, [4, 3], have) is have and layer_caps("labor", 1000, 5000, 3, [4, 3], have) is have
    # another number of layers: fresh
    assert _skb(layer_caps("stream", 1000, 5000, 10, [4], have)) == [(10, 81, 5000)]


def test_multinomial_floor_lifts_k_and_the_next_layers_s():
    have = [dict(S=10, C=1000, K=12, B=5000), dict(S=12, C=1000, K=14, B=5000)]
    # K0 = max(12, 4 + 10) = 14 -> S1 = 14 -> K1 = max(14, 3 + 14) = 17
    for kind in ("multinomial", "multinomial_replace"):
        assert _skb(layer_caps(kind, 1000, 5000, 10, [4, 3], have)) == [(10, 14, 5000), (14, 17, 5000)]
    # the host draw: K0 = 4 + 10 + 64 = 78 -> S1 = 78 -> K1 = 3 + 78 + 64 = 145; capped by V = 100
    assert _skb(layer_caps("multinomial_host", 1000, 5000, 10, [4, 3], have)) == [(10, 78, 5000), (78, 145, 5000)]
    assert _skb(layer_caps("multinomial_host", 100, 5000, 10, [4, 3], have)) == [(10, 78, 5000), (78, 100, 5000)]
    assert have[0]["K"] == 12 and have[1]["S"] == 12                            # (pure)
    assert layer_caps("stream", 1000, 5000, 10, [4, 3], have) is have          # (a Poisson layer's K has no floor)
    wide = [dict(S=10, C=1000, K=14, B=5000), dict(S=20, C=1000, K=30, B=5000)]
    assert layer_caps("multinomial", 1000, 5000, 10, [4, 3], wide) is wide     # nothing to lift


def test_static_caps():
    mx = [dict(K=20, B=30, E=100), dict(K=40, B=2000)]
    # K = int(1.5 * 20) + 256 = 286, B = 3 * 30 + 4096 = 4186, E = min(5000, 150 + 65536), X = min(4186, 45 + 2048);
    # then S = 286: K = 60 + 256, B = min(5000, 6000 + 4096), E = min(5000, 7500 + 65536), X = min(5000, 3000 + 2048)
    caps = static_caps("stream", 1000, 5000, 10, [4, 3], mx)
    assert caps == [dict(S=10, C=1000, K=286, B=4186, E=5000, X=2093), dict(S=286, C=1000, K=316, B=5000, E=5000, X=5000)]
    assert static_caps("labor", 1000, 5000, 10, [4, 3], mx) == caps
    # E under |E|
    assert static_caps("stream", 1000, 10 ** 6, 10, [4], mx)[0]["E"] == 65686
    # the margins; K capped by V
    assert _skb(static_caps("stream", 300, 5000, 10, [4, 3], mx, 2.0, 1.0)) == [(10, 296, 4126), (296, 300, 5000)]
    # device-drawn multinomial: K = f + S exactly
    for kind in ("multinomial", "multinomial_replace"):
        caps = static_caps(kind, 1000, 5000, 10, [4, 3], mx)
        assert _skb(caps) == [(10, 14, 4186), (14, 17, 5000)] and [c["X"] for c in caps] == [2093, 5000]
    assert _skb(static_caps("multinomial", 12, 5000, 10, [4, 3], mx)) == [(10, 12, 4186), (12, 12, 5000)]
    # neighbor layers: B = S * f exactly, capped by |E| without replacement; X follows B
    for kind in ("neighbor", "wneighbor"):
        caps = static_caps(kind, 1000, 5000, 10, [4, 3], mx)
        assert _skb(caps) == [(10, 286, 40), (286, 316, 858)] and [c["X"] for c in caps] == [40, 858]
        assert _skb(static_caps(kind, 1000, 100, 10, [4, 3], mx)) == [(10, 286, 40), (286, 316, 100)]
        assert _skb(static_caps(kind, 1000, 5000, 10, [-1, 3], mx)) == [(10, 286, 4186), (286, 316, 858)]      # f < 0: the margin rule
    assert _skb(static_caps("neighbor_replace", 1000, 100, 10, [4, 3], mx)) == [(10, 286, 40), (286, 316, 858)]
    assert static_caps("neighbor_replace", 2 * 10 ** 9, 100, 10 ** 9, [4], [dict(K=1, B=1)])[0]["B"] == 2 ** 31 - 1
