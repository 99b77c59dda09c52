"""OBCA local subproblem on the GPU: batched SQP (csrc/piadmm_obca.hip) behind
``piadmm_obca_solve`` (include/piadmm.h).

Mirrors the vehicle side of ``OBCAOptimizer`` (Distributed_planner/decentralized/optimizer.py):
``local_initialize`` + ``local_build_model`` + ``local_generate_constrain`` +
``local_generate_variable`` + ``local_generate_object`` + ``local_solve`` (:40-201) become one
record per (vehicle, ADMM iterate) and one batched call; ``bar_state`` keeps the reference's
arrays (``Z_bar``, ``A``, ``b``, ``lamb_bar``, ``lamb_ij``, ``local_x``, :351-373) and
``iterate_next_state`` (:337-344) shifts them.

Record layout (float64, ``REC`` per problem) -- what the reference's local NLP reads:
  init 5 | ref 8x5 (ref_traj[veh][t_step + k], also the initial X guess) | A_o 7x4x2 | b_o 7x4 |
  lamb_ij_o 7x4 (the other vehicle's bar_state slots) | lamb_bar 7x9 | Z_bar 7x9 |
  rho, min_dis, max_x, max_y, r, q, prob, max_iter | pad
Output (float64, ``OUT`` per problem): X 8x5 | U 7x2 | Lambda 7x4 | y_a 7 | y_b 7x2 | y_n 7 |
  y_x 7x5 | pi 7x5 | y_u 14 | y_l 28 | cost | pad;  status / SQP iterations / QP steps (int32 x 3).
"""
from __future__ import annotations

from .._lib import DELAY_PAR, DUAL_PAR, FEEDBACK_PAR, FLEET_PAR, NOISE_PAR, STATS_EDGES, STATS_WORST  # noqa: F401
from .model import *  # noqa: F401,F403
from .attach import *  # noqa: F401,F403
from .feedback import *  # noqa: F401,F403
from .stats import *  # noqa: F401,F403
from .tenant import *  # noqa: F401,F403
from .loop import *  # noqa: F401,F403
from .ledger import *  # noqa: F401,F403
from .batch import *  # noqa: F401,F403
from .planner import *  # noqa: F401,F403
from .device import *  # noqa: F401,F403
from .attach import _DUAL_DEFAULT  # noqa: F401
from .feedback import _FEEDBACK_DEFAULT, _PHILOX_M, _PHILOX_W, _U32, _plant_rhs  # noqa: F401
from .model import (_E_LB, _E_LIJ, _E_LX, _E_PAR, _EO_COST, _EO_DRES, _EO_LBN, _EO_YBND, _EO_YEQ,  # noqa: F401
                    _EO_YIN, _EO_Z, _EO_ZB, _FLEET_INTS, _O_AO, _O_BO, _O_INIT, _O_LB, _O_LIJ, _O_PAR, _O_REF, _O_ZB,
                    _box_vertex, _per_scenario, _spec)
from .planner import _scenario_refs, _spec_of  # noqa: F401
from .stats import _stats_call, _stats_edges, _stats_first  # noqa: F401
from .tenant import _TENANT_SHAPES, _tenant_row_check  # noqa: F401
