"""hydrodl2_amd -- MI355X-native HBV forward/backward time-stepper.

Drop-in for the model-plugin API of mhpi/hydrodl2 for ONE hot path: the HBV
per-day recurrence, its parameter prep, ensemble mean and unit-hydrograph
routing, forward and adjoint, as hand-written HIP kernels for gfx950 behind the
C ABI of include/hbvx.h.  See DESIGN.md.
"""
from hydrodl2_amd.api import available_models, available_modules, load_model, load_module
from hydrodl2_amd.sensitivity import jvp_batch, parameter_jacobian
from hydrodl2_amd.lstm import lstm_jvp_batch
from hydrodl2_amd.hourly_jvp import hourly_jvp_batch
from hydrodl2_amd.adj_jvp import adj_jvp_batch, adj_parameter_jacobian
from hydrodl2_amd.calibrate import calibrate, lm_step, normal_equations
from hydrodl2_amd.uncertainty import covariance_factor, parameter_covariance, predictive_variance
from hydrodl2_amd.population import (population_cost, population_joint_stats, population_period_stats, population_score,
                                     population_search, population_stats)
from hydrodl2_amd.population_fdc import population_fdc_score, population_fdc_stats
from hydrodl2_amd.adj_population import (adj_population_cost, adj_population_period_stats, adj_population_search,
                                         adj_population_stats)

from hydrodl2_amd.population_events import population_event_score, population_event_stats
from hydrodl2_amd.hourly_population import hourly_population_columns, hourly_population_stats
from hydrodl2_amd.hourly_fdc import hourly_fdc_score, hourly_population_fdc_stats
from hydrodl2_amd.ensemble import (EnsembleState, ensemble_forecast, ensemble_record, ensemble_step,
                                   particle_filter)
from hydrodl2_amd.enkf import enkf_filter, enkf_update
from hydrodl2_amd.hourly_events import (flood_events, hourly_event_score, hourly_population_event_stats,
                                        hourly_routing_search)

__version__ = "0.1.0"

__all__ = ["__version__", "available_models", "available_modules", "load_model", "load_module", "jvp_batch",
           "parameter_jacobian", "lstm_jvp_batch", "hourly_jvp_batch", "adj_jvp_batch", "adj_parameter_jacobian",
           "normal_equations", "lm_step", "calibrate", "parameter_covariance", "covariance_factor", "predictive_variance",
           "population_cost", "population_search", "population_stats", "population_score", "population_joint_stats",
           "population_period_stats", "population_fdc_stats", "population_fdc_score", "population_event_stats",
           "population_event_score",
           "adj_population_cost", "adj_population_stats", "adj_population_period_stats", "adj_population_search",
           "hourly_population_stats", "hourly_population_columns", "flood_events", "hourly_population_event_stats",
           "hourly_event_score", "hourly_routing_search", "hourly_population_fdc_stats", "hourly_fdc_score",
           "EnsembleState", "ensemble_record", "ensemble_step", "particle_filter", "ensemble_forecast",
           "enkf_update", "enkf_filter"]
