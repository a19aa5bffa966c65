// Bayesian negative-binomial (overdispersed count) regression with normal(0, s) priors on the intercept and
// the coefficients and a gamma prior on the dispersion phi (var = mu + mu^2 / phi).
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  int<lower=0> y[N];
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> phi;
}
model {
  alpha ~ normal(0, 2.5);
  beta ~ normal(0, 1);
  phi ~ gamma(2, 0.5);
  y ~ neg_binomial_2_log(alpha + x * beta, phi);
}
