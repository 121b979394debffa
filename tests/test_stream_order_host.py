"""CPU tier of the stream-order tests: the catalogue of tests/stream_order.py stays complete.

Every prototype of include/gs_abi.h whose parameter list ends in ``gs_stream_t stream)`` promises to launch everything on that
stream; tests/test_gpu_stream_order.py holds each of them to it on a stream whose inputs arrive late.  A new entry point fails
here until it has a case -- or one of the few exemptions, with its reason."""
import re

import stream_order as so

N_TODAY = 62

# what may never be exempt: the frame's forward and backwards, the losses, the optimizer steps, the exposure kernels
NEVER_EXEMPT = re.compile(r"^(gs_frame_forward$|gs_frame_backward|gs_loss_|gs_adam_|gs_exposure_)")


def test_the_header_parse_finds_the_stream_taking_prototypes():
    names = so.stream_entry_points()
    assert len(names) == len(set(names))
    assert len(names) >= N_TODAY, names
    for known in ("gs_world2camera", "gs_draw_backward", "gs_sort_pairs_bits", "gs_frame_forward", "gs_frame_async_wait",
                  "gs_frame_backward_adam_pose", "gs_loss_l1_ssim_weighted", "gs_exposure_backward", "gs_icp_step"):
        assert known in names
    # size queries, debug views and the handle's create / destroy take no stream
    for other in ("gs_frame_workspace_bytes", "gs_frame_async_create", "gs_frame_debug_views", "gs_last_error"):
        assert other not in names


def test_every_stream_taking_entry_point_has_a_case_or_a_reason():
    names = so.stream_entry_points()
    covered = {n for c in so.CASES for n in c.covers}
    missing = [n for n in names if n not in covered and n not in so.EXEMPT]
    assert not missing, f"no stream-order case covers {missing}: add one to tests/stream_order.py (CASES)"
    both = sorted(covered & set(so.EXEMPT))
    assert not both, f"{both} are exempt and covered: drop the exemption"


def test_neither_table_names_a_function_the_header_lacks():
    names = set(so.stream_entry_points())
    for c in so.CASES:
        assert c.covers, c.name
        assert not set(c.covers) - names, (c.name, sorted(set(c.covers) - names))
    assert not set(so.EXEMPT) - names, sorted(set(so.EXEMPT) - names)


def test_the_exemptions_are_few_and_never_the_hot_path():
    assert so.EXEMPT_MAX == 6 and len(so.EXEMPT) <= so.EXEMPT_MAX
    for name, reason in so.EXEMPT.items():
        assert not NEVER_EXEMPT.search(name), f"{name} may not be exempt: build its case"
        assert reason and "\n" not in reason, name


def test_the_cases_are_well_formed():
    names = [c.name for c in so.CASES]
    assert len(names) == len(set(names))
    for c in so.CASES:
        assert callable(c.build)
        assert c.synchronising is None or '"' in c.synchronising, f"{c.name}: quote the sentence that says the call waits"
