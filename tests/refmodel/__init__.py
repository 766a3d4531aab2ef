"""The float64 reference model of the queries, the cases a CPU suite and its GPU twin share, and the GPU harness: what the tests
import instead of each other.  A test file is never a library.

Layers, each importing downward only:
  records, tolerances                                   numpy alone
  rays -> spheres -> moves -> recover -> sandwich       the model: nothing of the product package
  visible, draw_batches, debug_lines                    the render references
  slabs, slab_cases                                     the sharded broadphase's stages in numpy, and the inputs of their tests
  *_cases                                               seeded generators and hand-worked tables; the package for dtypes and make_* only
  island_cases, obstacle_cases                          scenes per routing class of the solvers, and the kernels' routing restated in numpy
  boxbox64, boxbox_cases                                the box-box narrowphase as float64 geometry (numpy alone) with its sandwich checker; a pose pair per detector branch
                                                        and a tick sequence per branch of the manifold cache, classes read off the oracle's trace
  trigger_events, trigger_cases                         ProcessTriggerEvents in numpy; a scene per route and edge of the trigger pass, the oracle's driver
  device, *_device                                      the only modules that open a World; no *_cpu test reaches them
"""
import pytest

# the checkers' bare asserts keep pytest's introspection outside test_*.py: registered before any submodule is imported
pytest.register_assert_rewrite("refmodel.boxbox64", "refmodel.boxbox_cases", "refmodel.device", "refmodel.draw_batches", "refmodel.edge_cases", "refmodel.layout_cases", "refmodel.layout_device", "refmodel.move_cases",
                               "refmodel.obstacle_cases", "refmodel.recover_cases", "refmodel.sandwich", "refmodel.slab_cases", "refmodel.slabs", "refmodel.sphere_cases", "refmodel.trigger_cases", "refmodel.trigger_events", "refmodel.visible")
