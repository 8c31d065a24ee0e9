"""options_model_amd -- MI355X-native hot path of Levicoz/Options-model.

American-option Monte-Carlo pricing (GBM / Heston path generation -> Longstaff-Schwartz
backward induction -> discounted mean) as hand-written HIP kernels for gfx950 behind a C ABI
(include/omc.h, lib/libomc.so), with the reference's Python call surface kept as a drop-in:

    from options_model_amd import price_american_option           # north-star facade
    from options_model_amd import AdvancedOptionPricer, RNGManager   # options_model_3.py surface
    from options_model_amd.compat import Options_model, options_model_2   # v1 / v2 surfaces

Nothing here touches the GPU at import time.
"""
from ._ffi import OmcError, Context, default_context, device_count, load_library  # noqa: F401

__all__ = ["OmcError", "Context", "default_context", "device_count", "load_library"]


def __getattr__(name):
    # lazy: keep `import options_model_amd` cheap and free of side effects
    if name in ("price_american_option", "PriceResult", "price_european_option", "price_american_greeks", "GreeksResult",
                "price_barrier_option", "BarrierResult", "price_american_bounds", "BoundsResult", "price_american_chain",
                "ChainResult", "price_bermudan_option", "exercise_dates", "price_american_dividends", "DividendResult", "price_american_jumps", "JumpResult",
                "price_american_basket", "BasketResult", "price_american_basket_bounds", "BasketBoundsResult",
                "price_american_basket_greeks", "BasketGreeksResult", "price_american_bounds_heston",
                "HestonBoundsResult", "price_asian_option", "price_bermudan_bounds", "bounds_exercise_dates",
                "price_american_bounds_checked", "price_american_bounds_jumps", "JumpBoundsResult",
                "price_american_bounds_dividends", "DividendBoundsResult", "price_barrier_bounds",
                "BarrierBoundsResult", "price_american_dividend_greeks", "DividendGreeksResult",
                "price_american_chain_bounds", "ChainBoundsResult", "price_american_jump_greeks",
                "JumpGreeksResult", "price_american_chain_greeks", "ChainGreeksResult", "price_bermudan_greeks"):
        from . import api
        return getattr(api, name)
    if name in ("AdvancedOptionPricer", "RNGManager", "BlackScholesGreeks", "welford_batch_update",
                "monte_carlo_price_streaming", "compute_curve_worker_enhanced"):
        from . import pricer
        return getattr(pricer, name)
    raise AttributeError(name)
