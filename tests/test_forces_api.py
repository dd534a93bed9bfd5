"""CPU-side checks of the energy-and-force interface (gmp_amd.second_order,
gmp_amd.energy_and_forces) and of the yardstick the GPU tests compare against: the fp64 oracle's
forces equal central differences of its energy."""
import pytest
import torch


def test_public_names_exist():
    import gmp_amd
    from gmp_amd import ops
    assert callable(gmp_amd.energy_and_forces)
    assert gmp_amd.second_order is ops.second_order
    assert "second_order" in gmp_amd.__all__ and "energy_and_forces" in gmp_amd.__all__


def test_context_nests_and_restores():
    import gmp_amd
    from gmp_amd import ops
    assert not ops.second_order_enabled()
    with gmp_amd.second_order():
        assert ops.second_order_enabled()
        with gmp_amd.second_order():
            assert ops.second_order_enabled()
        assert ops.second_order_enabled()
        with pytest.raises(ValueError):
            with gmp_amd.second_order():
                raise ValueError("boom")
        assert ops.second_order_enabled()
    assert not ops.second_order_enabled()
    with pytest.raises(KeyError):
        with gmp_amd.second_order():
            raise KeyError("boom")
    assert not ops.second_order_enabled()


def test_context_refuses_compile_tracing(monkeypatch):
    import gmp_amd
    from gmp_amd import ops
    monkeypatch.setattr(ops, "compiling", lambda: True)
    with pytest.raises(NotImplementedError):
        with gmp_amd.second_order():
            pass
    assert not ops.second_order_enabled()


def test_oracle_forces_equal_central_differences():
    """The yardstick itself: on the k-chains pair in fp64, -autograd.grad(E, pos) of the oracle
    equals central differences of E to 1e-6 of the force scale."""
    from gmp_amd.graph import Batch, collate, create_kchains
    from oracle import schnet as osch
    torch.manual_seed(3)
    b = collate(create_kchains(4))
    ref = osch.SchNetModel(hidden_channels=64, num_filters=128, num_layers=4, num_gaussians=50,
                           cutoff=10, out_dim=1)
    with torch.no_grad():
        ref.embedding.weight.normal_()
    ref = ref.double()

    def energy(pos):
        return ref(Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=b.num_graphs)).sum()

    pos = b.pos.double().requires_grad_(True)
    (g,) = torch.autograd.grad(energy(pos), pos)
    F = -g
    h = 1e-4
    fd = torch.zeros_like(F)
    with torch.no_grad():
        for i in range(pos.shape[0]):
            for k in range(3):
                d = torch.zeros_like(pos)
                d[i, k] = h
                fd[i, k] = -(energy(pos + d) - energy(pos - d)) / (2 * h)
    scale = F.abs().max().item()
    assert scale > 0
    assert (F - fd).abs().max().item() <= 1e-6 * scale
