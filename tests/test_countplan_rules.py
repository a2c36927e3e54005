"""The plan rule of the k <= 7 count whose workgroups pull their work (csrc/vk_countplan.h, pull_plan): the grid and the
bound on a sample's helpers as a function of the workgroups the device holds, the samples and their parts."""
import pytest

from countplan_emul_lib import pull_plan, tail_helpers


def test_the_grid_is_what_is_resident_and_never_more_than_the_batch_can_use():
    assert pull_plan(512, 1000, 16)[0] == 512
    assert pull_plan(512, 100, 20)[0] == 512
    assert pull_plan(512, 600, 2)[0] == 512      # more samples than workgroups: every workgroup owns several in turn
    assert pull_plan(512, 3, 2)[0] == 6          # a workgroup's wavefronts want a chunk each: samples * parts at most
    assert pull_plan(512, 1, 2)[0] == 2
    assert pull_plan(608, 1000, 16)[0] == 608    # (another device)
    assert pull_plan(512, 0, 4) == (0, 0) and pull_plan(0, 5, 4) == (0, 0) and pull_plan(512, 5, 0) == (0, 0)


def test_a_small_batch_fills_the_device_from_the_start():
    """owners + helpers cover the grid: nsamples * (1 + helpers) >= grid, without a whole spare round of helpers"""
    for resident, nsamples, parts in ((512, 32, 64), (512, 100, 20), (512, 3, 2), (512, 7, 40), (608, 100, 20), (512, 511, 4)):
        grid, helpers = pull_plan(resident, nsamples, parts)
        assert nsamples * (1 + helpers) >= grid, (resident, nsamples, parts)
        assert helpers == max(tail_helpers(), -(-grid // nsamples) - 1), (resident, nsamples, parts)
    assert pull_plan(512, 32, 64) == (512, 15)
    assert pull_plan(512, 100, 20) == (512, 5)
    assert pull_plan(512, 3, 2) == (6, 1)


def test_many_samples_keep_the_tail_bound():
    t = tail_helpers()
    assert t >= 1
    assert pull_plan(512, 1000, 16) == (512, t)
    assert pull_plan(512, 512, 16) == (512, t)
    assert pull_plan(512, 100000, 2) == (512, min(t, 1))


@pytest.mark.parametrize("resident", (512, 608))
def test_a_sample_never_gets_more_helpers_than_it_has_parts_to_feed(resident):
    for nsamples in (1, 2, 5, 201, 600, 5000):
        for parts in (1, 2, 3, 5, 16, 512):
            grid, helpers = pull_plan(resident, nsamples, parts)
            if parts == 1:
                assert (grid, helpers) == (0, 0)   # samples of one part: the static launch, a workgroup each
                grid, helpers = pull_plan(resident, nsamples, parts, 3)   # ... unless a bound is forced:
                assert helpers == 0   # a sample of one part is its owner's alone, one flush
            assert 1 <= grid <= min(resident, nsamples * parts)
            assert helpers <= parts - 1
    assert pull_plan(512, 201, 5) == (512, 2)   # one 40 MB sample among 200 small ones (choose_parts: 5 parts)


def test_a_forced_bound_is_capped_the_same_way():
    assert pull_plan(512, 1000, 16, 7) == (512, 7)
    assert pull_plan(512, 1000, 16, 0) == (512, 0)
    assert pull_plan(512, 1000, 4, 7) == (512, 3)
    assert pull_plan(512, 600, 1) == (0, 0) and pull_plan(512, 600, 1, 0) == (512, 0) and pull_plan(512, 600, 1, 5) == (512, 0)
