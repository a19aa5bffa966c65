// Gamma regression with the log link, normal(0, s) priors on alpha and beta and a gamma(2, 0.5) prior on shape.
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  vector<lower=0>[N] y;
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> shape;
}
model {
  alpha ~ normal(0, 10);
  beta ~ normal(0, 2.5);
  shape ~ gamma(2, 0.5);
  y ~ gamma(shape, shape ./ exp(alpha + x * beta));
}
