"""MI355X-native HMC/NUTS sampler for The Economist's 2020 poll model (hot path only).

Layout: csrc/ (HIP kernels + the C ABI of include/potus_hmc.h), sampler.py (host mirror of the
reference's `$sample()` / `rstan::extract()` surface), dataprep.py / synthetic.py (Stan data
lists), diagnostics.py (R-hat / ESS), outcomes.py (joint election outcomes: EV histogram, tipping point), monitor.py (the posterior summary table), scenario.py (conditional forecasts, covariance of the state scores), timeline.py (run dates as the data sets of one handle), crossval.py (exact K-fold and leave-future-out cross-validation), sensitivity.py (prior settings as the data sets of one handle, and their distance from the baseline), _abi.py (ctypes structs).
"""
from . import _abi  # noqa: F401
from .sampler import (Handle, Optimum, PotusError, PotusModel, StanFit, backtest_scores, check_convergence, device_diagnostics, device_diagnostics_of_block,  # noqa: F401
                      load_library, posterior_summary, run_many, sampling)
from . import outcomes  # noqa: F401,E402  (the module; its outcomes() is also available as joint_outcomes)
from .outcomes import Outcomes, outcomes_of_block  # noqa: F401,E402
from .outcomes import outcomes as joint_outcomes  # noqa: F401,E402
from . import monitor  # noqa: F401,E402  (the module; its monitor() is also available as monitor_table)
from .monitor import Monitor, monitor_of_block  # noqa: F401,E402
from .monitor import monitor as monitor_table  # noqa: F401,E402
from . import scenario  # noqa: F401,E402  (the module; its scenario() is also available as conditional_forecast)
from .scenario import Scenario, scenario_of_block  # noqa: F401,E402
from .scenario import scenario as conditional_forecast  # noqa: F401,E402
from . import sensitivity  # noqa: F401,E402  (prior sensitivity by refit: grid(), fit(), Grid; Handle.set_datasets_grid is the call beneath)
from .sampler import SCALE_NAMES, ecdf_distance_device  # noqa: F401,E402
