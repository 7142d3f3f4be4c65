"""CPU suite: ``fit``'s ``train_step`` keyword is checked before anything touches a device."""
import pytest


def test_fit_refuses_an_unknown_train_step():
    from bliss_gnn_amd import fit
    with pytest.raises(ValueError, match="train_step"):
        fit.fit(None, None, None, None, None, train_step="bogus")
    import inspect
    assert inspect.signature(fit.fit).parameters["train_step"].default == "eager"
