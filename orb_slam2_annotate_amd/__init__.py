"""MI355X-native ORB front-end: the ORBextractor / ORBmatcher hot path of ORB-SLAM2 as
hand-written HIP (gfx950) behind a C-ABI (include/orbfe.h).  This package is the host-side
mirror of the reference's class interface; it binds liborbfe.so with ctypes and has no
compute of its own (and no CPU fallback)."""
from ._lib import KP_DTYPE, OrbfeError, LIB_PATH  # noqa: F401
from .extractor import ORBextractor, gaussian_blur7, resize_linear, set_blur_pass_order  # noqa: F401
from .matcher import ComputeStereoMatches, FeatureVector, FrameView, ORBmatcher, ResidentFrame  # noqa: F401
from .vocabulary import ORBVocabulary, synthetic_vocabulary_arrays, write_synthetic_vocabulary, write_vocabulary_text  # noqa: F401
from .map_points import MapPoints, camera_pose, motion_model_mode, sim3_leg, track_with_motion_model  # noqa: F401
from .optimizer import (bundle_adjustment, local_bundle_adjustment, optimize_sim3, optimize_sim3_multi,  # noqa: F401
                        pose_optimization, pose_optimization_batch, sim3_to_Rts)
from .local_mapping import KeyFrameCamera, triangulate_matches, triangulate_matches_multi, triangulated_points_select  # noqa: F401
from .relocalization import (PnPsolver, pnp_ransac, pnp_ransac_multi, pnp_refine_multi,  # noqa: F401
                             pnp_sets_from_draws, pnp_solve_multi)
from .loop_closing import (Sim3Solver, correct_loop_points, correct_loop_sim3s, gba_propagate_keyframes,  # noqa: F401
                           gba_update_points, sim3_legs, sim3_max_iterations, sim3_ransac, sim3_ransac_multi,
                           sim3_triples_from_draws)
from .initializer import (Initializer, initializer_normalize, initializer_ransac, initializer_ransac_multi,  # noqa: F401
                          initializer_reconstruct, initializer_reconstruct_multi, initializer_sets_from_draws)
from .keyframe_database import KeyFrameDatabase, bow_arrays, group_candidates  # noqa: F401
from .observation_graph import ObservationGraph  # noqa: F401
from .tracking import STEREO_ALL, STEREO_KEYFRAME, STEREO_TEMPORAL, count_close_points, stereo_points_select  # noqa: F401
from .ingest import (ComputeDistinctiveDescriptors, ComputeImageBounds, ComputeStereoFromRGBD,  # noqa: F401
                     Rectifier, UndistortKeyPoints, cvtColorToGray, initUndistortRectifyMap, undistortPoints)  # noqa: F401
